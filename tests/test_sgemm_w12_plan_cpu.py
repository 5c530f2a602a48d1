"""Host-side checks of the staging-wave sgemm kernel's forms of twelve multiplying waves (256 x 192 | 192 x 256 tiles): what the planner takes and refuses by tile string,
and that every size of sgemm-ops-full plans to rectangles that tile c exactly.  Nothing is compiled and no device is needed."""
import os
import re

import pytest

from boda_amd import rtc as R
from boda_amd.op import UnsupErr, parse_op, read_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not hasattr(R._lib, "bodahip_explain_plan"), reason="the C ABI exposes no plan query")


def sg(M, N, K):
    return parse_op(f"(str_vals=(type=sgemm,func_name=hip_sgemm),nda_vals=(a=(dims=(K={K},M={M})),b=(dims=(K={K},N={N})),c=(dims=(M={M},N={N}))))")


def test_w12_tile_strings():
    q = R.explain_plan(sg(1536, 1536, 1536), tile="256x192x16x4x3x4x1x32x2x3")
    assert q.startswith("bodahip_sgemm_big_f32 256x192x16_w4x3_p2_stg ") and "-DBKS=16 -DPF=2 -DTBI=256 -DTBJ=192 -DWI=4 -DWJ=3 -DMINW=4" in q and "NSTG" not in q, q
    q = R.explain_plan(sg(1536, 1536, 1536), tile="192x256x16x3x4x4x1x32x4x3x3")
    assert q.startswith("bodahip_sgemm_big_f32 192x256x16_w3x4_p4_stg ") and "-DTBI=192 -DTBJ=256 -DWI=3 -DWJ=4 -DMINW=4 -DNSTG=3" in q, q
    assert "-DNSTG=4" in R.explain_plan(sg(1536, 1536, 1536), tile="256x192x16x4x3x4x1x32x2x3x4")
    # the ten-field strings of the other forms keep their option lists (their cached code objects stay valid)
    assert R.explain_plan(sg(2048, 2048, 2048), tile="64x64x16x2x2x4x1x32x2x3").split(" ", 2)[2].split() == "-DBKS=16 -DPF=2 -DTBI=64 -DTBJ=64 -DWI=2 -DWJ=2 -DMINW=4".split()


@pytest.mark.parametrize("tile", ["256x192x8x4x3x4x1x32x2x3",       # BKS 8: 8 x 48 float4 units are no multiple of the 256 staging threads
                                  "320x192x16x5x3x4x1x32x2x3",      # 5 x 3 waves
                                  "256x192x32x4x3x4x1x32x2x3",      # four stages of 32 x (256 + 192 + 8) floats: 228 KB of LDS
                                  "256x192x32x4x3x4x1x32x2x3x3",    # ... and three: 171 KB
                                  "384x128x16x6x2x4x1x32x2x3",      # twelve waves, but not 4 x 3 | 3 x 4
                                  "256x192x16x4x3x8x1x32x2x3",      # a register budget of eight waves per SIMD: sixteen waves are four
                                  "256x192x16x4x3x4x1x32x2x3x5"])   # five LDS stages
def test_w12_malformed_tiles_rejected(tile):
    with pytest.raises(UnsupErr, match="unsupported staging-wave tile"):
        R.explain_plan(sg(1536, 1536, 1536), tile=tile)


def _rects(plan, M, N):
    if plan.startswith("parts="):
        return [(int(a), int(b), int(c), int(d)) for a, b, c, d in re.findall(r"\[(\d+)\+(\d+),(\d+)\+(\d+)\]:", plan)]
    m = re.match(r"rows<(\d+):", plan)
    if m: return [(0, int(m.group(1)), 0, N), (int(m.group(1)), M - int(m.group(1)), 0, N)]
    return [(0, M, 0, N)]


def test_every_list_size_plans_to_rectangles_that_tile_c():
    ops = read_ops(os.path.join(ROOT, "tests", "golden", "ops", "sgemm-ops-full.txt"))
    assert len(ops) == 17
    for op in ops:
        g = op.sgemm_geom(); M, N = g["M"], g["N"]
        plan = R.explain_plan(sg(M, N, g["K"]))
        rs = _rects(plan, M, N)
        if plan.startswith("parts="): assert len(rs) == int(plan.split()[0][6:]), plan
        assert all(r > 0 and c > 0 and m0 + r <= M and n0 + c <= N for m0, r, n0, c in rs), plan
        assert sum(r * c for _, r, _, c in rs) == M * N, plan
        for i, (m0, r, n0, c) in enumerate(rs):
            for m1, r1, n1, c1 in rs[i + 1:]:
                assert m0 + r <= m1 or m1 + r1 <= m0 or n0 + c <= n1 or n1 + c1 <= n0, (plan, "two rectangles overlap")
