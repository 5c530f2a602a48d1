"""-m gpu: bench.py as the driver runs it.  (1) `python bench.py --gpus 2` launches ITSELF under torch.distributed.run (one process per GPU) and
prints one JSON line from rank 0; on the one-GPU test box BENCH_SAME_GPU=1 puts both ranks on GPU 0 over gloo, which exercises the whole N>1
branch -- sharded data generation, the one-time weight broadcast (no silent fallback), barrier / max-over-ranks timing -- with the HIP kernels
doing the arithmetic.  (2) the --full N=1 line carries the AlexNet / NiN conv-ops legs under `conv_ops`.  (3) a plain N=1 run does the headline only, and
--dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "OMP_NUM_THREADS", "OMP_WAIT_POLICY"):   # (the OMP bounds are the test session's, tests/conftest.py: the driver runs bench.py without them)
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, lines


@pytest.mark.parametrize("workload", ["nin-net", "nin", "sgemm-ops-full"])
def test_bench_launches_itself_for_two_ranks(workload):
    args = ["--gpus", "2", "--workload", workload, "--steps", "1", "--warmup", "0", "--settle-ms", "0"] + ([] if workload == "sgemm-ops-full" else ["--batch", "8"])
    r, lines = _bench(args, {"BENCH_SAME_GPU": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])          # exactly one JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert "broadcast once" in out["config"]["weights"] and "failed" not in out["config"]["weights"]
    assert out["config"]["rccl_ranks"] == 2
    assert "cpu_baseline" not in out                                        # rank 0 at N=1 only


@pytest.mark.parametrize("args", [["--workload", "nin-net", "--batch", "128"],                                           # BASELINE configs[3] per GPU: 1024 images over 8
                                  ["--workload", "googlenet", "--dtype", "bf16", "--layout", "nhwc", "--graph", "--batch", "64"]],   # configs[4] per GPU: 512 over 8
                         ids=["config4_nin-net_b128", "config5_googlenet_b64_bf16"])
def test_eight_ranks_at_the_per_gpu_shapes_of_configs_4_and_5(args):
    """The command the driver runs on an 8-GPU node (`bench.py --gpus 8 ...`), end to end once: eight ranks, each at the per-GPU shape of the BASELINE config, here
    all on GPU 0 over gloo.  Whole-job value = 8 x the per-rank units over the slowest rank's time; weights broadcast once from rank 0."""
    r, lines = _bench(["--gpus", "8", "--steps", "2", "--warmup", "1", "--settle-ms", "0"] + args, {"BENCH_SAME_GPU": "1"}, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["scaling"] == "weak" and out["value"] > 0 and out["config"]["rccl_ranks"] == 8
    assert "broadcast once" in out["config"]["weights"] and "failed" not in out["config"]["weights"]
    assert "parallelism" in out["config"] and "x8" in out["config"]["parallelism"]
    if "nin-net" in args:
        assert "batch 128/GPU" in out["config"]["workload"] and out["images_per_s"] > 0


def test_the_documented_scale_command_on_two_ranks():
    """README's SCALE command -- `bench.py --gpus N --workload nin-net --batch 128 --graph` (config 4, weak scaling, no collective on the data path) -- with two ranks on
    GPU 0 (round-5 verdict item 7): two RCCL-side ranks, the broadcast weights digest-equal on both, and the two-rank aggregate within 2x of the one-process rate (both ranks
    share one GPU here, so the aggregate is about the single rate: what is checked is that nothing serialises or stalls beyond that)."""
    common = ["--workload", "nin-net", "--batch", "128", "--graph", "--steps", "3", "--warmup", "1", "--settle-ms", "50", "--no-cpu-baseline"]
    r1, l1 = _bench(common)
    assert r1.returncode == 0 and len(l1) == 1, r1.stderr[-2000:]
    one = json.loads(l1[0])
    r2, l2 = _bench(["--gpus", "2"] + common, {"BENCH_SAME_GPU": "1"}, timeout=900)
    assert r2.returncode == 0 and len(l2) == 1, r2.stderr[-3000:]
    two = json.loads(l2[0])
    assert two["n_gpus"] == 2 and two["config"]["rccl_ranks"] == 2 and two["config"]["weights_digest_equal"] is True
    assert two["images_per_s"] > 0 and one["images_per_s"] > 0
    assert 0.5 * one["images_per_s"] < two["images_per_s"] < 2.0 * one["images_per_s"], (one["images_per_s"], two["images_per_s"])


def test_world_size_mismatch_is_an_error():
    r, lines = _bench(["--gpus", "2", "--steps", "1"], {"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode == 2 and not lines


def test_default_line_carries_conv_ops():
    r, lines = _bench(["--full", "--steps", "2", "--warmup", "1", "--settle-ms", "100"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["config"]["workload"].startswith("test/sgemm-ops-full.txt") and out["dtype"] == "f32"
    assert out["roofline"]["bound"] == "mfma" and out["cpu_baseline"]["value"] > 0
    co = out["conv_ops"]
    for nm, n_layers in (("alexnet", 8), ("nin", 12)):
        assert len(co[nm]["per_op"]) == n_layers and co[nm]["value"] > 0 and 0 < co[nm]["roofline"]["frac"] <= 1
    h = co["nin"]["roofline"]["hbm_frac_1x1"]                             # cccp1 / cccp2 (AI 24): priced against HBM as well
    assert h["layers"] == [1, 2] and 0 < h["frac"] <= 1
    tol = co["tolerance_mode"]                                              # op_tune hip_exact=0 beside the bit-exact default
    assert set(tol) == {"alexnet", "nin"} and all(0 < v["frac"] <= 1 and v["value"] > 0 for v in tol.values())
    cf = out["configs"]                                                     # BASELINE configs[3] / [4] as legs of the same line
    assert set(cf) >= {"config4_nin-net_b128_f32", "config5_googlenet_b64_bf16_nhwc", "config5_resnet50_b64_bf16_nhwc", "config5_googlenet_b64_bf16_nhwc_independent",
                       "config5_resnet50_b64_bf16_nhwc_independent", "config5_googlenet_b64_bf16_nhwc_independent_multi"}
    for nm in ("googlenet", "resnet50"):     # the edge-free graph replays the same kernels: never slower than the chain by more than noise, and it says what it is
        ind, ch = cf[f"config5_{nm}_b64_bf16_nhwc_independent"], cf[f"config5_{nm}_b64_bf16_nhwc"]
        assert "no edges" in ind["launch"] and "chain" in ch["launch"] and ind["ms_per_step"] < 1.15 * ch["ms_per_step"]
    assert all("error" not in v and v["value"] > 0 and 0 < v["roofline"]["frac"] <= 1 for v in cf.values()), cf


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """`bench.py --steps K --warmup W` without --full: the headline line only (nothing that takes runs of its own), K timed steps; --dump-outputs writes
    every op's output of the last step -- whole where small, a fixed sample where large -- and both are the oracle's products of the same inputs."""
    import numpy as np
    import bench
    from oracle import boda_oracle as bo
    d = tmp_path / "dump"
    r, lines = _bench(["--steps", "3", "--warmup", "1", "--settle-ms", "0", "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "TFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert not {"conv_ops", "configs", "cpu_baseline", "compile", "ref_style_gpu", "summary"} & set(out) and out["roofline"]["kernel"] is None
    ops = bench.sgemm_full_ops()
    files = sorted(os.listdir(d))
    assert files == [f"op{i:02d}_c.npy" for i in range(len(ops))]
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    cap = bench.DUMP_BUDGET_ELEMS // len(ops)
    for i, op in enumerate(ops):
        n = op.sgemm_geom()["M"]
        if n > 1024:
            continue
        got = np.load(d / f"op{i:02d}_c.npy")
        assert got.dtype == np.float32
        want = bo.sgemm(bo.gen_sgemm_a(n, n), bo.gen_sgemm_b(n, n))
        if n * n <= cap:
            assert np.array_equal(got, want), n
        else:
            idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n * n, cap, replace=False))
            assert got.shape == (cap,) and np.array_equal(got, want.reshape(-1)[idx]), n
