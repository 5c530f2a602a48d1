"""Grouped convolution without a GPU: the op layer (group on a Convolution / BckConv, its geometry and refusals), the annotators and their refusals, the native
table's rows and plans, be=cpu's three grouped functions bit for bit against be=cpu's ungrouped functions on the slices (tests/conv_grp_ref.py), be=cpu against
float64 under the bounds the ungrouped functions are held to, and the cnn_op_info counts."""
import numpy as np
import pytest

from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import (BCONV_GRP_FUNCS, CONV_GRP_FUNC, NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_bck_conv_grp_annotations, add_codegen_annotations,
                             annotate_k1_chain, bconv_filts_biases_func_op, bf16_operands, filts_kmajor_func_op, fuse_f32_pool, fuse_zero_if_in_non_pos, k1_chain_applies, pipe_func_args)
from boda_amd.cnn_op_info import OpInfoToLatex
from boda_amd.op import RtErr, UnsupErr, parse_op
from boda_amd.rtc import make_rtc

from conv_grp_ref import CASE_IDS, CASES, bck_op, bits_equal, conv_op, grouped_funcs, mrd, rand_ins, run_func, sliced, torch_twin
from test_bck_conv_cpu import FILTS_MRD

FWD_MRD = 2e-4   # the forward tests' bound against float64 (the reference's max-rel-diff tolerance, src/rtc_prof.cc:161)


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the op layer
def test_geometry_of_a_grouped_op():
    g = conv_op(2, 3, 12, 96, 9, 11, 5, 2, 2).conv_geom()
    assert (g["G"], g["CG"], g["OCG"], g["C"], g["OC"]) == (3, 4, 32, 12, 96)
    g = bck_op(3, 19, 19, 19, 10, 9, 3, 2, 1).bck_conv_geom()
    assert (g["G"], g["CG"], g["OCG"]) == (19, 1, 1)
    assert "G" not in conv_op(2, 1, 12, 96, 9, 11, 5, 2, 2).conv_geom()                      # group=1 written out
    assert "G" not in conv_op(2, 1, 12, 96, 9, 11, 5, 2, 2, group_field=False).conv_geom()


def test_geometry_refusals_name_the_three_numbers():
    ok = conv_op(2, 2, 12, 8, 9, 9, 3, 1, 1).to_str()
    for bad, nums in ((ok.replace("group=(tn=uint32_t,v=2)", "group=(tn=uint32_t,v=5)"), ("group=5", "in.chan=12", "filts.out_chan=8")),     # divides neither
                      (ok.replace("group=(tn=uint32_t,v=2)", "group=(tn=uint32_t,v=3)"), ("group=3", "in.chan=12", "filts.out_chan=8")),     # OC % g
                      (ok.replace("in_chan=6", "in_chan=12"), ("group=2", "in.chan=12", "filts.in_chan=12"))):                                # filts not C/g
        with pytest.raises(RtErr) as e:
            parse_op(bad)
        assert all(n in str(e.value) for n in nums), str(e.value)
    with pytest.raises(RtErr) as e:   # without group the existing message stays word for word
        parse_op(ok.replace("group=(tn=uint32_t,v=2),", ""))
    assert str(e.value) == "conv: filts.in_chan != in.chan (groups are not on this path)"
    with pytest.raises(RtErr):
        parse_op(bck_op(2, 2, 12, 8, 9, 9, 3, 1, 1).to_str().replace("group=(tn=uint32_t,v=2)", "group=(tn=uint32_t,v=5)"))


def test_annotations():
    case = CASES[0]
    fc, fi, fb, ff = grouped_funcs(case)
    assert fc.get_func_name() == CONV_GRP_FUNC == "hip_conv_grp" and fc.get_u32("conv_has_relu") == 1
    assert tuple(f.get_func_name() for f in (fi, fb, ff)) == BCONV_GRP_FUNCS == ("hip_bconv_in_grp", "hip_bconv_biases", "hip_bconv_filts_grp")
    assert [f.get_func_name() for f in add_bck_conv_grp_annotations(bck_op(*case), OpTune())] == list(BCONV_GRP_FUNCS)
    assert NATIVE_ARGS["hip_conv_grp"] == NATIVE_ARGS["hip_conv"] and NATIVE_ARGS["hip_bconv_in_grp"] == NATIVE_ARGS["hip_bconv_in"]
    assert NATIVE_ARGS["hip_bconv_filts_grp"] == NATIVE_ARGS["hip_bconv_filts"]
    for f in (fc, fi, ff):
        assert rtc_mod.func_args(f) == pipe_func_args(f) == NATIVE_ARGS[f.get_func_name()]
    t = "1x1x16x2x2x1x2"
    ti, tb, tf = add_bck_conv_annotations(bck_op(*case), OpTune(hip_tile=t))
    assert ti.str_vals["hip_tile"] == tf.str_vals["hip_tile"] == t and "hip_tile" not in tb.str_vals
    for foreign in ("64x128x16x2x2", "64x128x16x2x2x2"):   # a pipe-wide tile written for the ungrouped functions passes a grouped op by
        assert all("hip_tile" not in f.str_vals for f in add_bck_conv_annotations(bck_op(*case), OpTune(hip_tile=foreign)))
        assert "hip_tile" not in add_codegen_annotations(conv_op(*case), OpTune(hip_tile=foreign)).str_vals
    assert add_codegen_annotations(conv_op(*case), OpTune(hip_tile="1x2x1x2x2x1x1")).str_vals["hip_tile"] == "1x2x1x2x2x1x1"
    with pytest.raises(RtErr):
        add_bck_conv_grp_annotations(bck_op(2, 1, 6, 10, 7, 6, 3, 1, 1), OpTune())   # no group > 1: the ungrouped annotator's op


def test_group_1_is_no_group(cpu):
    case = (2, 1, 6, 10, 7, 6, 3, 1, 1)
    ins = rand_ins(case, 3)
    for mk, ann in ((conv_op, lambda o: (add_codegen_annotations(o, OpTune()),)), (bck_op, lambda o: add_bck_conv_annotations(o, OpTune()))):
        with_g, without = ann(mk(*case)), ann(mk(*case, group_field=False))
        assert [f.get_func_name() for f in with_g] == [f.get_func_name() for f in without]
        assert not any(n.endswith("_grp") for n in (f.get_func_name() for f in with_g))
        for a, b in zip(with_g, without):
            assert rtc_mod.explain_plan(a) == rtc_mod.explain_plan(b)
            assert bits_equal(run_func(cpu, a, ins)[0], run_func(cpu, b, ins)[0])


def test_every_other_function_and_option_refuses_by_name():
    cv, bk = conv_op(*CASES[3]), bck_op(*CASES[3])
    for tune in (OpTune(hip_dtype="bf16"), OpTune(hip_dtype="bf16", hip_layout="nhwc"), OpTune(hip_algo="winograd"), OpTune(k1conv=1), OpTune(tconv=1), OpTune(ipconv=1),
                 OpTune(use_culibs=1)):
        for f, op in ((add_codegen_annotations, cv), (add_bck_conv_annotations, bk)):
            with pytest.raises(UnsupErr, match="group"):
                f(op, tune)
    fc, fi, fb, ff = grouped_funcs(CASES[3])
    with pytest.raises(UnsupErr, match="group"):
        bconv_filts_biases_func_op(bk, OpTune())
    for f in (fi, ff):
        with pytest.raises(UnsupErr, match="group"):
            bf16_operands(f)
    with pytest.raises(UnsupErr, match="group"):
        fuse_zero_if_in_non_pos(fi)
    plain = add_codegen_annotations(conv_op(2, 1, 64, 32, 7, 7, 1, 1, 0, group_field=False), OpTune())
    assert not k1_chain_applies(plain, fc) and not k1_chain_applies(fc, plain)
    with pytest.raises(UnsupErr, match="group"):
        annotate_k1_chain(fc, plain, 1, 1)
    with pytest.raises(UnsupErr, match="group"):
        filts_kmajor_func_op(fc)
    with pytest.raises(UnsupErr, match="group"):
        fuse_f32_pool(fc.copy(), fc.get_dims("in"), (2, 2), (2, 2))
    assert filts_kmajor_func_op(plain).to_str() == "(str_vals=(func_name=hip_conv_filts_kmajor,type=Convolution),nda_vals=())"
    for fn in ("hip_conv", "hip_conv_bf16", "hip_conv_winograd", "cudnn_conv"):   # the backend's own refusal, whoever wrote the function name
        bad = fc.copy(); bad.str_vals["func_name"] = fn
        with pytest.raises(UnsupErr, match="group=4"):
            rtc_mod.explain_plan(bad)
    for fn in ("hip_bconv_in", "hip_bconv_filts", "hip_bconv_filts_biases"):
        bad = fi.copy(); bad.str_vals["func_name"] = fn
        with pytest.raises(UnsupErr, match="group=4"):
            rtc_mod.explain_plan(bad)
    assert rtc_mod.explain_plan(fb).startswith("bodahip_bconv_biases")   # the bias gradient knows no groups


# ---- the native table and the planner
def test_table_rows():
    t = rtc_mod.native_funcs()
    for n, member, typ in (("hip_conv_grp", 1, "Convolution"), ("hip_bconv_in_grp", 2, "BckConv"), ("hip_bconv_filts_grp", 3, "BckConv")):
        r = t[n]
        assert r["family"] == "conv_grp" and r["member"] == member and tuple(r["types"]) == (typ,) and not r["flags"] and not r["opt"]
        assert set(r["be"]) == {"hip", "cpu"} and r["multi_dev"] == "one_device"


def test_plans():
    fc, fi, _, ff = grouped_funcs(CASES[2])
    # the planner chooses the form from the op alone: AlexNet conv2 shrunk (OCG = 40, CG = 48) is matrix ground, 32 x 32 x 2 blocks
    assert rtc_mod.explain_plan(fc).startswith("bodahip_conv_grp_mfma 32x256x32_w1x4 ") and "-DFORM=1 -DCG=48 -DOCG=40" in rtc_mod.explain_plan(fc) and "-DMT=32" in rtc_mod.explain_plan(fc)
    assert rtc_mod.explain_plan(fi).startswith("bodahip_bconv_in_grp_mfma ")
    assert rtc_mod.explain_plan(ff).startswith("bodahip_bconv_filts_grp_mfma 32x64x32_w1x1")
    for case, form, m16 in ((CASES[3], "direct", False), (CASES[1], "mfma", False), (CASES[0], "direct", False), (CASES[5], "direct", False), (CASES[7], "direct", False),
                            ((32, 32, 128, 128, 56, 56, 3, 1, 1), "direct", False), ((32, 32, 512, 512, 14, 14, 3, 1, 1), "mfma", True)):
        plans = [rtc_mod.explain_plan(f).split() for f in (grouped_funcs(case)[0], grouped_funcs(case)[3])]   # (the grouped 1x1 reduces over 8 terms: direct; 16 out_chans a group: 16 x 16 x 4 blocks)
        assert all(pl[0].endswith("_" + form) and ("_m16" in pl[1]) == m16 for pl in plans), (case, plans)
    p = rtc_mod.explain_plan(ff, tile="1x1x16x2x2x1x8")      # BI = 1 forces the direct form
    assert p.startswith("bodahip_bconv_filts_grp_direct 1x1x16_w2x2_s8 ") and "-DBK=16 -DKSL=8" in p
    p = rtc_mod.explain_plan(ff, tile="16x32x12x1x1x1x3")   # BI > 1 the matrix form; 16 rows a wave: 16 x 16 x 4 blocks; three waves, the slices
    assert p.startswith("bodahip_bconv_filts_grp_mfma 16x32x12_w1x1_m16_s3 ") and "-DMT=16" in p and "-DKSL=3" in p
    assert rtc_mod.explain_plan(grouped_funcs(CASES[5])[0], tile="32x128x2x1x4x1x1").startswith("bodahip_conv_grp_mfma 32x128x2_w1x4 ")   # (a depthwise op forced onto the matrix form)
    big = grouped_funcs((32, 32, 32, 32, 112, 112, 3, 1, 1))[3]   # a depthwise layer with a long K: the planner slices it
    assert "_s" in rtc_mod.explain_plan(big).split()[1]
    assert "_s" in rtc_mod.explain_plan(grouped_funcs((256, 2, 384, 256, 13, 13, 3, 1, 1))[3]).split()[1]   # and AlexNet conv5's filter gradient in the matrix form
    for foreign in ("1x4x1x2x2", "64x128x16x2x2", "64x128x16x2x2x2x1x32x2x2"):   # not the family's seven-field form (a pipe-wide hip_conv tile): the planner decides
        assert rtc_mod.explain_plan(fc, tile=foreign) == rtc_mod.explain_plan(fc)
    for bad in ("1x3x1x2x2x1x1", "1x1x1x2x2x1x2", "1x4x1x1x1x1x1", "48x128x2x1x4x1x1", "32x128x3x1x4x1x1", "32x128x2x1x4x1x2", "16x64x2x1x4x1x1"):
        with pytest.raises(UnsupErr):   # three outputs per thread; slices on the forward; one wave; 48 rows a wave; an odd BK; slices on the forward; BK 2 on 16 x 16 x 4
            rtc_mod.explain_plan(fc, tile=bad)
    assert rtc_mod.explain_plan(grouped_funcs(CASES[5])[3], tile="1x1x4x2x2x1x300").startswith("bodahip_bconv_filts_grp_direct 1x1x4_w2x2_s300 grid=23 ")   # a thread per (out_chan, in_chan) pair and slice
    assert rtc_mod.explain_plan(grouped_funcs(CASES[5])[3], tile="1x1x4x2x2x1x300").endswith(" | bodahip_bconv_filts_grp_slab_sum")   # slices: the slabs' sum is a second launch
    assert "slab_sum" not in rtc_mod.explain_plan(grouped_funcs(CASES[5])[3], tile="1x1x4x2x2x1x1")
    eleven = grouped_funcs((2, 2, 4, 4, 23, 23, 11, 4, 0))[3]   # 121 taps: more than the direct form holds in registers
    assert rtc_mod.explain_plan(eleven).startswith("bodahip_bconv_filts_grp_mfma ")
    with pytest.raises(UnsupErr, match="49 taps"):
        rtc_mod.explain_plan(eleven, tile="1x1x32x2x2x1x1")
    for bad in ("1x1x32x2x2x1x1025", "32x32x32x1x1x1x17", "32x32x32x1x4x1x2", "64x64x32x1x1x1x8"):   # too many slices (direct, matrix); waves that are no slices; slabs beyond the LDS
        with pytest.raises(UnsupErr):
            rtc_mod.explain_plan(ff, tile=bad)


# ---- be=cpu: the definition, bit for bit, and float64
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cpu_grouped_is_ungrouped_on_slices(cpu, case):
    ins = rand_ins(case, 5)
    fc, fi, fb, ff = grouped_funcs(case)
    for which, f in (("fwd", fc), ("in", fi), ("filts", ff)):
        assert bits_equal(run_func(cpu, f, ins)[0], sliced(cpu, case, ins, which)), (case, which)
    want_b = run_func(cpu, add_bck_conv_annotations(bck_op(case[0], 1, case[3], case[3], *case[4:], group_field=False), OpTune())[1], ins)[0]
    assert bits_equal(run_func(cpu, fb, ins)[0], want_b)   # the bias gradient: the function of any op with these out_grad_loss dims


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cpu_against_float64(cpu, case):
    ins = rand_ins(case, 5)
    fc, fi, _, ff = grouped_funcs(case)
    o, gi, gw = torch_twin(case, ins)
    got = [run_func(cpu, f, ins)[0] for f in (fc, fi, ff)]
    print(case, [mrd(a, b) for a, b in zip(got, (o, gi, gw))])
    assert mrd(got[0], o) < FWD_MRD and mrd(got[1], gi) < 2e-4 and mrd(got[2], gw) < FILTS_MRD


def test_cpu_forward_without_relu(cpu):
    case = CASES[0]
    ins = rand_ins(case, 5)
    f = grouped_funcs(case)[0].copy(); f.nda_vals["conv_has_relu"].v = (0,)
    got = run_func(cpu, f, ins)[0]
    assert got.min() < 0 and mrd(got, torch_twin(case, ins, relu=False)[0]) < FWD_MRD


def test_cpu_refuses_vars_that_disagree(cpu):
    fc = grouped_funcs(CASES[0])[0]
    ins = rand_ins(CASES[0], 5)
    ins["filts"] = np.zeros((10, 6, 3, 3), np.float32)   # ungrouped filters for a grouped op
    with pytest.raises(RtErr):
        run_func(cpu, fc, ins)


# ---- cnn_op_info
def test_info_counts():
    for case in (CASES[2], CASES[5]):
        B, g, C, OC, H, W, k, s, p = case
        op = conv_op(*case)
        geo = op.conv_geom()
        flops = 2 * B * OC * geo["OH"] * geo["OW"] * (C // g) * k * k
        assert op.flops() == flops and bck_op(*case).flops() == 2 * flops
        nbytes = 4 * (B * C * H * W + B * OC * geo["OH"] * geo["OW"] + OC * (C // g) * k * k + OC)
        assert op.algo_bytes() == nbytes
        tl = OpInfoToLatex(op)
        assert (tl.flops, tl.bytes, tl.K) == (flops, nbytes, (C // g) * k * k)
    plain = conv_op(2, 1, 96, 80, 13, 13, 5, 1, 2, group_field=False)
    assert plain.flops() == 2 * conv_op(*CASES[2]).flops()   # two groups: half the work of the ungrouped layer
