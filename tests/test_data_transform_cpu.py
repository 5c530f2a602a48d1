"""The input transform without a GPU: the numpy twin of hip_data_transform held to hand-computed answers, the function on be=cpu against the twin byte for byte over
the sampled shape product (tests/data_ref.py), every refusal with its sentence, the table row and the Python mirrors, InputTransform's plans (known answers, spread),
prototxt.transform_spec, and the two drivers on be=cpu."""
import os

import numpy as np
import pytest

import data_ref as D
from boda_amd import prototxt
from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import DATA_OP_FUNCS, NATIVE_ARGS, data_transform_func_op, pipe_func_args
from boda_amd.input_pipe import InputTransform, fmix32, plan_word
from boda_amd.op import OP_INFO, Dims, Op, RtErr, UnsupErr, read_ops
from boda_amd.rtc import make_rtc

F, U8, U32 = np.float32, np.uint8, np.uint32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "data-ops.txt")


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- 1. the twin itself, by hand
def test_twin_mirrored_crop_by_hand():
    src = np.array([1, 2, 3, 4], U8).reshape(1, 1, 4, 1)     # 1 x 1 x 4 x 1: one image, one row of four pels, one channel
    out = D.data_transform_np(src, np.array([[0, 1, 1, 0]], U32), np.zeros(1, F), 1.0, (1, 3), "hwc")
    assert out.reshape(-1).tolist() == [4.0, 3.0, 2.0]
    assert D.data_transform_np(src, np.array([[0, 1, 0, 0]], U32), np.zeros(1, F), 1.0, (1, 3), "hwc").reshape(-1).tolist() == [2.0, 3.0, 4.0]


def test_twin_takes_the_per_pel_mean_at_the_source_column():
    src = np.array([10, 20, 30, 40], U8).reshape(1, 1, 1, 4)     # planar
    mean = np.array([1, 2, 3, 4], F).reshape(1, 1, 4)
    plain = D.data_transform_np(src, np.array([[0, 1, 0, 0]], U32), mean, 1.0, (1, 3), "chw").reshape(-1)
    assert plain.tolist() == [18.0, 27.0, 36.0]     # 20 - 2, 30 - 3, 40 - 4
    mirrored = D.data_transform_np(src, np.array([[0, 1, 1, 0]], U32), mean, 1.0, (1, 3), "chw").reshape(-1)
    assert mirrored.tolist() == [36.0, 27.0, 18.0]     # the mean moves with the pel: NOT 40 - 2, 30 - 3, 20 - 4


def test_twin_clamps_and_rounds_twice():
    src = np.arange(12, dtype=U8).reshape(1, 3, 4, 1)
    big = D.data_transform_np(src, np.array([[0xFFFFFFFF, 7, 0x80000000, 5]], U32), np.zeros(1, F), 1.0, (2, 2), "hwc")
    assert big.reshape(-1).tolist() == [7.0, 6.0, 11.0, 10.0]     # offsets clamped to (1, 2); 0x80000000 mirrors
    d = F(F(200) - F(0.1))
    out = D.data_transform_np(np.array([200], U8).reshape(1, 1, 1, 1), np.zeros((1, 4), U32), np.array([0.1], F), 0.017, (1, 1), "hwc")
    assert out.reshape(-1)[0] == F(d * F(0.017)) and float(d) != 200 - 0.1


# ---- 2. the function on be=cpu
CASES = D.function_cases()


def test_case_list_holds_the_corners_and_the_product():
    assert 55 <= len(CASES) <= 65
    assert {c["chan"] * c["ch"] * c["cw"] * c["B"] for c in CASES[:12]} == {1, 135, 3900}
    for key, vals in (("chan", {1, 3, 4}), ("cw", {1, 5, 63, 64, 65}), ("ch", {1, 3}), ("dw", {0, 1, 6}), ("dh", {0, 2}), ("B", {1, 3, 5}), ("layout", {"hwc", "chw"}), ("pel", {0, 1}),
                      ("scale", set(D.SCALES))):
        assert {c[key] for c in CASES} == vals, key
    rows = D.plan_rows(2, 6)
    assert {(0, 0, 0), (0, 6, 1), (2, 0, 1), (2, 6, 0)} <= {r[:3] for r in rows} and any(r[2] == 2 for r in rows) and any(r[2] == 0x80000000 for r in rows)
    assert any(r[0] == 0xFFFFFFFF for r in rows) and any(r[:2] == (3, 7) for r in rows) and all(r[3] not in (0, 1) for r in rows)
    sd, md, src, mean, plans = D.case_data(CASES[8])     # a 3900-element corner
    assert set(src.reshape(-1).tolist()) == set(range(256))
    assert len({tuple(r) for p in plans for r in p.tolist()}) == len(rows) and all(len({tuple(r) for r in p.tolist()}) == len(p) for p in plans)


@pytest.mark.parametrize("c", CASES, ids=D.case_id)
def test_function_is_the_twin(cpu, c):
    D.check_case(cpu, c)


def test_means_hold_the_special_values():
    seen = set()
    for c in CASES:
        m = D.case_data(c)[3].reshape(-1)
        seen |= {"nan"} if np.isnan(m).any() else set()
        seen |= {"-0"} if np.any((m == 0) & np.signbit(m)) else set()
        seen |= {"inf"} if np.any(m == np.inf) else set()
        seen |= {"-inf"} if np.any(m == -np.inf) else set()
        seen |= {"rounds"} if np.any(m == F(0.1)) else set()
    assert seen == {"nan", "-0", "inf", "-inf", "rounds"}


def test_realistic_case(cpu):
    D.check_realistic(cpu)


def test_bad_ops_are_refused_with_their_sentences(cpu):
    D.check_bad_ops(cpu)


def test_bad_calls_are_refused_and_larger_vars_run(cpu):
    D.check_bad_calls(cpu)


# ---- 3. the table row and the mirrors
def test_table_row():
    table = rtc_mod.native_funcs()
    r = table["hip_data_transform"]
    assert r == {"family": "data", "member": 1, "types": ("DataTransform",), "flags": (), "be": ("hip", "cpu"), "multi_dev": "on_shards", "opt": (), "why": ""}
    names = list(table)
    assert names[-4:] == ["hip_data_transform", "hip_accuracy", "hip_eval_accum", "hip_bn_fold"]     # in front of the eval rows, the table's last three
    assert DATA_OP_FUNCS == {"DataTransform": ("hip_data_transform",)}
    assert NATIVE_ARGS["hip_data_transform"] == (("src", "IN"), ("plan", "IN"), ("mean", "IN"), ("out", "OUT"))
    assert OP_INFO["DataTransform"] == (("src", "plan", "mean"), ("out",), ("scale",))
    assert rtc_mod.func_args(Op({"type": "DataTransform", "func_name": "hip_data_transform"}, {})) == NATIVE_ARGS["hip_data_transform"]


def test_golden_ops():
    ops = read_ops(GOLD)
    assert {(o.data_geom()["layout"], o.data_geom()["mean_form"]) for o in ops} == {("hwc", "chan"), ("hwc", "chan:y:x"), ("chw", "chan"), ("chw", "chan:y:x")}
    for o in ops:
        assert o.get_func_name() == "hip_data_transform"
        assert rtc_mod.func_args(o) == pipe_func_args(o) == NATIVE_ARGS["hip_data_transform"]
        g = o.data_geom()
        again = data_transform_func_op(o.get_dims("src"), (g["ch"], g["cw"]), o.get_dims("mean"), g["scale"])
        assert again.to_str() == o.to_str()


def test_func_op_refuses_a_bad_source():
    with pytest.raises(RtErr, match="src must be uint8_t img:y:x:chan or img:chan:y:x"):
        data_transform_func_op(Dims.make("float", img=1, y=2, x=2, chan=1), (1, 1), Dims.make("float", chan=1), 1.0)
    with pytest.raises(RtErr, match="the crop 3 x 1 is larger than the source 2 x 2"):
        data_transform_func_op(Dims.make("uint8_t", img=1, y=2, x=2, chan=1), (3, 1), Dims.make("float", chan=1), 1.0)


# ---- 4. the plan
def test_plan_known_answers():
    assert fmix32(0) == 0 and [plan_word(7, k) for k in range(3)] == [0x18C9AEC4, 0x36DEB503, 0xC80D16A4]
    xf = InputTransform((256, 256), crop=227, mirror=True, seed=7)     # H - ch + 1 = W - cw + 1 = 30
    p = xf.plan("train", 0, 8)
    assert p.dtype == U32 and p.shape == (8, 4)
    assert [tuple(r[:3]) for r in p.tolist()] == [(10, 25, 0), (10, 10, 0), (15, 22, 0), (12, 20, 0), (24, 5, 1), (27, 18, 0), (3, 29, 0), (23, 18, 0)]
    assert np.array_equal(xf.plan("train", 3, 4), p[3:7])     # a plan is a function of the global image index
    assert not np.array_equal(xf.plan("train", 8, 8), p)     # two consecutive batches differ
    assert not np.array_equal(InputTransform((256, 256), crop=227, mirror=True, seed=8).plan("train", 0, 8), p)


def test_test_plan_is_the_centre_crop():
    assert InputTransform((256, 256), crop=227, mirror=True).plan("test", 5, 3).tolist() == [[14, 14, 0, 0]] * 3     # an odd margin, 29
    assert InputTransform((10, 13), crop=6, mirror=True).plan("test", 0, 2).tolist() == [[2, 3, 0, 0]] * 2          # margins 4 and 7
    assert InputTransform((9, 9)).plan("test", 0, 1).tolist() == [[0, 0, 0, 0]] and InputTransform((9, 9)).plan("train", 0, 2)[:, :2].tolist() == [[0, 0], [0, 0]]


@pytest.mark.parametrize("seed", [0, 1, 12345, 0xFFFFFFFF])
def test_plan_spread(seed):
    """4096 images over 5 x 7 offsets: every (y, x, mirror) triple occurs, every offset's count lies within 15 % of uniform, the mirror share within 0.5 +- 0.03."""
    xf = InputTransform((14, 16), crop=10, mirror=True, seed=seed)     # rectangular sources need a square crop: 14 - 10 + 1 = 5, 16 - 10 + 1 = 7
    p = xf.plan("train", 0, 4096)
    assert p[:, 0].max() == 4 and p[:, 1].max() == 6 and set(p[:, 2].tolist()) == {0, 1} and not p[:, 3].any()
    assert len({tuple(r) for r in p[:, :3].tolist()}) == 70
    # an offset's count: how many images get that y_off (of 5), that x_off (of 7).  The issue's own figures -- worst count 9 % off, worst mirror share 0.011 off -- are
    # these marginals' (the 35 cells of 117 images each scatter by a fifth under any uniform hash)
    for col, n_off in ((0, 5), (1, 7)):
        cnt = np.bincount(p[:, col], minlength=n_off)
        uni = 4096 / n_off
        print("seed %d: %s counts %d .. %d of %.1f (%.1f %% .. %.1f %%)" % (seed, "yx"[col], cnt.min(), cnt.max(), uni, 100 * (cnt.min() / uni - 1), 100 * (cnt.max() / uni - 1)))
        assert cnt.min() >= 0.85 * uni and cnt.max() <= 1.15 * uni
    print("seed %d: mirror share %.4f" % (seed, p[:, 2].mean()))
    assert abs(p[:, 2].mean() - 0.5) <= 0.03
    off = InputTransform((14, 16), crop=10, mirror=False, seed=seed).plan("train", 0, 4096)
    assert not off[:, 2].any() and np.array_equal(off[:, :2], p[:, :2])     # mirror=False gives no mirror and the same offsets


def test_check_plan():
    xf = InputTransform((14, 16), crop=10)
    ok = np.array([[4, 6, 1, 77], [0, 0, 0x80000000, 0]], U32)
    assert xf.check_plan(ok).dtype == U32 and np.array_equal(xf.check_plan(ok, 2), ok)
    with pytest.raises(RtErr, match=r"image 1: y_off=5 is beyond the range 0 \.\. 4"):
        xf.check_plan(np.array([[4, 6, 0, 0], [5, 0, 0, 0]], U32))
    with pytest.raises(RtErr, match=r"image 0: x_off=7 is beyond the range 0 \.\. 6"):
        xf.check_plan(np.array([[0, 7, 0, 0]], U32))
    with pytest.raises(RtErr, match="integer array of shape"):
        xf.check_plan(np.zeros((2, 3), U32))
    with pytest.raises(RtErr, match=r"shape \(3, 4\)"):
        xf.check_plan(ok, 3)
    with pytest.raises(RtErr, match="outside uint32"):
        xf.check_plan(np.array([[0, 0, -1, 0]], np.int64))


def test_input_transform_refusals_and_means():
    with pytest.raises(RtErr, match="both mean_value and mean"):
        InputTransform((8, 8), mean_value=1.0, mean=np.zeros((3, 8, 8), F))
    with pytest.raises(RtErr, match="crop=9 is larger than the source 8 x 12"):
        InputTransform((8, 12), crop=9)
    with pytest.raises(RtErr, match="mean must be chan:y:x at the source size 8 x 8"):
        InputTransform((8, 8), crop=4, mean=np.zeros((3, 4, 4), F))
    with pytest.raises(RtErr, match="layout must be"):
        InputTransform((8, 8), layout="nhwc")
    with pytest.raises(RtErr, match="2 mean values for 3 channels"):
        InputTransform((8, 8), mean_value=(1.0, 2.0)).mean_array(3)
    assert InputTransform((8, 8)).mean_array(3).tolist() == [0.0, 0.0, 0.0]     # neither mean: zeros
    assert InputTransform((8, 8), mean_value=5).mean_array(3).tolist() == [5.0] * 3     # Caffe's broadcast of one value
    assert InputTransform((8, 8), mean_value=(1, 2, 3)).mean_array(3).tolist() == [1.0, 2.0, 3.0]
    xf = InputTransform((8, 9), crop=0, layout="chw")
    assert (xf.ch, xf.cw) == (8, 9) and xf.src_dims(2, 3) == Dims.make("uint8_t", img=2, chan=3, y=8, x=9)
    assert InputTransform((8, 9)).src_dims(2, 3) == Dims.make("uint8_t", img=2, y=8, x=9, chan=3)


# ---- 5. prototxt.transform_spec
NET = """
name: "n"
layer { name: "d_train" type: "Data" top: "data" top: "label" include { phase: TRAIN }
  transform_param { mirror: true crop_size: 227 mean_value: 104 mean_value: 117 mean_value: 123 scale: 0.017 } data_param { source: "x" batch_size: 32 } }
layer { name: "d_test" type: "Data" top: "data" top: "label" include { phase: TEST }
  transform_param { mirror: false crop_size: 224 mean_file: "mean.binaryproto" } }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 4 kernel_size: 3 } }
"""


def test_transform_spec():
    assert prototxt.transform_spec(NET, "train") == {"crop_size": 227, "mirror": True, "scale": 0.017, "mean_value": [104.0, 117.0, 123.0], "mean_file": ""}
    assert prototxt.transform_spec(NET, "test") == {"crop_size": 224, "mirror": False, "scale": 1.0, "mean_value": [], "mean_file": "mean.binaryproto"}
    bare = 'layer { name: "d" type: "Data" top: "data" }'
    for ph in ("train", "test"):     # Caffe's defaults; a layer without an include block serves both phases
        assert prototxt.transform_spec(bare, ph) == {"crop_size": 0, "mirror": False, "scale": 1.0, "mean_value": [], "mean_file": ""}
    assert [n for n, _ in prototxt.conv_ops(NET, 2)] == ["conv1"] and prototxt.conv_ops(NET, 2)[0][1].get_dims("in").sizes == (2, 3, 224, 224)     # conv_ops as before


def test_transform_spec_refusals():
    both = 'layer { name: "d" type: "Data" top: "data" transform_param { mean_file: "m" mean_value: 1 } }'
    with pytest.raises(RtErr, match="both mean_file and mean_value"):
        prototxt.transform_spec(both, "train")
    for key in ("force_color", "force_gray"):
        with pytest.raises(UnsupErr, match=key):
            prototxt.transform_spec('layer { name: "d" type: "Data" top: "data" transform_param { %s: true } }' % key, "test")
    assert prototxt.transform_spec('layer { name: "d" type: "Data" top: "data" transform_param { force_gray: false } }', "test")["crop_size"] == 0
    with pytest.raises(RtErr, match="no Data layer of the train phase"):
        prototxt.transform_spec('layer { name: "d" type: "Data" top: "data" include { phase: TEST } }', "train")
    with pytest.raises(RtErr, match="phase must be"):
        prototxt.transform_spec(NET, "TRAIN")


# ---- 6. the drivers on be=cpu
@pytest.mark.parametrize("name,iter_size", [("chain", 1), ("chain", 2), ("residual", 1)])
def test_step_is_the_step_on_the_twins_floats(cpu, name, iter_size):
    D.check_step(cpu, name, iter_size)


@pytest.mark.parametrize("name", ["chain", "residual"])
def test_call_deps_put_the_transform_in_front_of_datas_readers(cpu, name):
    D.check_call_deps(cpu, name)


@pytest.mark.parametrize("name", ["chain", "residual"])
def test_eval_pipe_uses_the_centre_plan(cpu, name):
    D.check_eval(cpu, name)


@pytest.mark.parametrize("name", ["chain", "residual"])
def test_training_is_undisturbed_by_evaluations(cpu, name):
    D.check_training_is_undisturbed(cpu, name)


def test_refusals_and_defaults(cpu):
    D.check_refusals_and_defaults(cpu)
