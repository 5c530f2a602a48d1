"""Seeded random-geometry sweeps of the training BatchNorm (kernels/bn_f32.hip: the hip_bn_*, hip_bnc_* and hip_bnf_* families), the full SoftmaxWithLoss
(kernels/loss_f32.hip), the solver family, the evaluation functions and the input transform on the MI355X, on the cases of tools/fuzz_step.py under the table of tests/test_step_fuzz_cpu.py, which holds the check_*_case functions and runs
them on be=cpu on these very cases.

  * bn: hip_bn_stats, hip_bn_fwd (relu 0 and 1), hip_bn_bck_sums, hip_bn_bck_in and hip_fan_out equal be=cpu and the numpy twin by bits on two lists of twelve geometries
    (the quad path: slabs above 1024 and 4096 elements, the host-made walk with step_pel = 0, with the carry, with step_img = 0 and on planes of 1024 pels, ragged last
    slabs, chains without an element, the planner's plan of three slabs; the element path: planes of 1, 2 and 3 pels over 64 images and more, odd planes above 1024 pels,
    slab edges inside a plane, C = 1, 255, 256, 257, N = 1), on data of three kinds; the in-place forms on two cases per path; bn_ref's float64 bounds on the `normal` cases
  * bnf: hip_bnf_prep, hip_bnf_bck and hip_bnf_bck_in, with their in-place forms, on the same lists by bits
  * bnc: the chunked chain on twelve cases (an empty chunk, a chunk of one image, chunks that do not divide the batch, a chunk of two or more slabs) by bits
  * loss: the three functions chained on two lists of twelve (HW 63 / 64 / 65; the pel form at C = 1, 31, 32, 33 and above 64; the wave form below, at and above 64
    channels; 256 pels and around; tensors of no whole quads; one quad across images; all pels ignored; an ignore_label that is a class): prob and loss_per_pel under
    loss_ref's bounds, loss, loss_state and in_grad_loss by bits against the twins and be=cpu on the GPU's own prob and loss_per_pel
  * solver: hip_solver_update under every form, hip_sgd_update, hip_grad_accum and hip_solver_update_acc on twelve drawn tensor lists (tens_num 1, 31, 32; a tensor of
    one chunk, of one chunk and 1 to 3 scalars, of less than a quad; no size a multiple of 4), hip_grad_sumsq + hip_grad_norm on twelve drawn call lists, three of them
    with about 300 partials (the second round of hip_grad_norm's lanes), the clip below, above and equal to the norm: bits against the twins and be=cpu
  * eval: hip_accuracy on twelve (B, C) draws with B % 4 and C % 64 both non-zero, logits from eight values and invalid labels; hip_eval_accum around 256 and 512 images
    under top_k 1, 2, C, C + 3; hip_bn_fold at C 1-600 on eval_ref's special values.  data: hip_data_transform on twelve drawn crops (cw 1, 2, 3; no whole quads; crop equal
    to source; both layouts and mean forms; every plan with a mirrored image whose x offset is clamped), bytes against the twin and be=cpu
Every launch: NaN-filled outputs, guard vars, inputs that keep their bits (the runners of bn_ref / loss_ref), the function's own kernel, for bodahip_bn_sum and the loss
kernels the grid of the plan restated in fuzz_step; every reducing call twice on the same workspace with the same bits.  The check_*_case functions are also what
tools/fuzz_step.py runs, in volume.

Measured on one MI355X (pytest --durations=0, the file alone; these kernels are specialised by a few -D values, not by geometry, so the build's code-object cache holds them
all): 12 tests in 5.3 s, test_solver_update 3.1 s (twelve tensor lists under eight forms, two backends and the twins), every other test below 0.4 s.  Largest observed
fractions of the bounds: bn out 0.891, dx 0.806, S1 0.052, scale_grad 0.057, bias_grad 0.041; loss prob 0.521 (pel) / 0.494 (wave), loss_per_pel 0.750.  No mismatch on these
lists, nor on tools/fuzz_step.py 50 1 all (650 cases, 15 s); with the `++img` of the quad path's carry in bodahip_bn_sum dropped, test_bn[bn_q], test_bnf[bn_q] and test_bnc fail
where every test of test_gpu_bn.py, test_gpu_bnc.py and test_gpu_freeze.py passes."""
import pytest

from boda_amd.rtc import make_rtc

from test_step_fuzz_cpu import (BN_LISTS, INPLACE, LOSS_LISTS, USED, WORST, acc_list, accum_list, bn_list, bnc_list, check_acc_case, check_accum_case, check_bn_case,
                                check_bnc_case, check_bnf_case, check_data_case, check_fold_case, check_loss_case, check_norm_case, check_solver_case, data_list, data_seed,
                                fold_list, loss_list, norm_list, solver_list)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


@pytest.mark.parametrize("key", list(BN_LISTS))
def test_bn(hip, cpu, key):
    path = "quad" if key == "bn_q" else "elem"
    before = USED.get(f"bn_sum {path} slabs>1", 0)
    for i, case in enumerate(bn_list(key)):
        check_bn_case(hip, cpu, case, data_seed(key, i), inplace=i in INPLACE[key])
    assert USED.get(f"bn_sum {path} slabs>1", 0) - before >= 2, USED   # bodahip_bn_sum ran with more than one slab on this load path


@pytest.mark.parametrize("key", list(BN_LISTS))
def test_bnf(hip, cpu, key):
    for i, case in enumerate(bn_list(key)):
        check_bnf_case(hip, cpu, case, data_seed(key, i))


def test_bnc(hip, cpu):
    for i, case in enumerate(bnc_list()):
        check_bnc_case(hip, cpu, case, data_seed("bnc", i))


@pytest.mark.parametrize("key", list(LOSS_LISTS))
def test_loss(hip, cpu, key):
    for i, case in enumerate(loss_list(key)):
        check_loss_case(hip, cpu, case)


def test_solver_update(hip, cpu):
    for i, case in enumerate(solver_list()):
        check_solver_case(hip, cpu, case, data_seed("solver", i))


def test_solver_norm(hip, cpu):
    for i, case in enumerate(norm_list()):
        check_norm_case(hip, cpu, case, data_seed("norm", i))


def test_eval(hip, cpu):
    for case in acc_list():
        check_acc_case(hip, cpu, case)
    for case in accum_list():
        check_accum_case(hip, cpu, case)
    for case in fold_list():
        check_fold_case(hip, cpu, case)


def test_data(hip, cpu):
    for c in data_list():
        check_data_case(hip, cpu, c)


def test_zz_report_worst_fractions_of_the_bounds():
    """Not a check of its own: prints what the sweeps above measured (run with -s) and the kernels they launched (test_bn asserts that bodahip_bn_sum ran with
    more than one slab on each load path)."""
    for name in sorted(WORST):
        print(f"largest observed fraction of the bound, {name}: {WORST[name]:.3f}")
    print("kernels used:", dict(sorted(USED.items(), key=lambda kv: -kv[1])))
    assert all(v <= 1.0 for v in WORST.values())
