"""bench.py's output contract and its CPU-side helpers (no GPU): the committed bench line under profiles/ carries every key the driver and
the tier brief ask for (metric / value / unit / ..., `roofline`, `cpu_baseline`), its numbers are mutually consistent, and the helpers
that fold the committed PMC table into the line read it the way DESIGN.md says."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ["bench.py", *args]
    try:
        import bench
        return bench, bench.parse()
    finally:
        sys.argv = argv


def _line(name="r06_bench.json"):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        return json.loads(fh.read().strip().splitlines()[-1])


def test_defaults_are_one_gpu_and_a_run_of_minutes():
    bench, a = _bench()
    assert a.gpus == 1 and a.steps == 20 and a.warmup == 5 and a.batch == 64 and a.points == 3000
    assert a.workload == "fusion_s8" and a.precision == "fp32x3" and a.graph == 1 and a.sync_bn == 1      # the headline precision meets north_star's tolerance
    legs = ("no_cpu_baseline", "no_kernel_timing", "no_fwd", "no_fp32_leg", "no_ffl", "no_b16", "no_predict", "no_host_feed")
    assert not a.full and a.dump_outputs is None and all(getattr(a, k) for k in legs)      # a plain run times the headline step only
    _, f = _bench("--full")
    assert not any(getattr(f, k) for k in legs)                                           # --full reports every leg
    _, f = _bench("--full", "--no-ffl")
    assert f.no_ffl and not any(getattr(f, k) for k in legs if k != "no_ffl")


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs: one float32 .npy per array (the loss float64); an array over its cap is written as the elements at fixed seeded positions,
    the same in every run, so that two builds compare element for element."""
    import types
    import numpy as np
    import torch
    bench, _ = _bench()
    m = torch.nn.Linear(3000, 400)                     # 1.2 M parameters: more than the parameter sample
    for p in m.parameters():
        p.grad = torch.full_like(p, 0.5)
    st = types.SimpleNamespace(model=m, out=torch.tensor(1.25), outputs=(torch.arange(12.0).view(3, 4), torch.ones(2, 2, dtype=torch.float64)))
    for d in ("a", "b"):
        bench.dump_outputs(st, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grads_sample.npy", "logits.npy", "loss.npy", "params_sample.npy", "perm.npy"]
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == (np.float64 if f == "loss.npy" else np.float32) and np.array_equal(a, b), f
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [1.25]
    assert np.array_equal(np.load(tmp_path / "a" / "logits.npy"), np.arange(12.0, dtype=np.float32).reshape(3, 4))
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    idx = np.sort(np.random.default_rng(0).choice(flat.size, size=bench.DUMP_PARAM_SAMPLE, replace=False))
    assert np.array_equal(np.load(tmp_path / "a" / "params_sample.npy"), flat[idx])
    assert (np.load(tmp_path / "a" / "grads_sample.npy") == 0.5).all()


def test_committed_bench_line_has_the_contract_keys_and_is_self_consistent():
    d = _line()
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert base["metric"].startswith(d["metric"]) and d["unit"] == "tiles/s"      # BASELINE names the N = 1/2/4/8 sweep and fwd ms/tile after it
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    # the headline precision is the one that meets north_star's tolerance, and the line carries its own measured error against the oracle
    assert d["precision"] == "fp32x3" and d["dtype"].startswith("f32") and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    e = d["fp32x3_vs_oracle"]
    assert e["logits_rel"] < 1e-3 and e["perm_rel"] < 1e-3 and e["argmax_agree"] == 1.0 and e["argmax_positions"] >= 770
    assert d["bf16_vs_oracle"]["logits_rel"] > 1e-3                                        # why bf16 is a sub-object and not `value`
    tiles = d["config"]["tiles_per_gpu"] * d["n_gpus"]
    assert abs(d["value"] - tiles / d["ms_per_step"] * 1e3) < 0.01 * d["value"]            # value = whole-job tiles / step time
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and (r["peak"] == 8000.0 or abs(r["peak"] - 2500.0 / 3.0) < 1.0)
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # achieved = algorithmic bytes (or FLOP) per launch / measured launch time: re-derive it from the line's own fields
    if r["bound"] == "hbm":
        assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 0.01 * r["achieved"]
    else:
        assert abs(r["achieved"] - r["algorithmic_flop_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e12) < 0.01 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] >= 0.9 * r["algorithmic_bytes_per_launch"]   # counter traffic cannot be below the algorithmic bytes
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["unit"] == d["unit"] and c["cores"] >= 1 and c["value"] > 0
    for key, dt_ in (("fp32_exact_mode", "f32"), ("bf16_mode", "bf16")):
        f = d[key]
        assert f["dtype"] == dt_ and f["value"] > 0 and abs(f["value"] - tiles / f["ms_per_step"] * 1e3) < 0.01 * f["value"]
    assert d["bf16_mode"]["value"] > d["value"] > d["fp32_exact_mode"]["value"]
    p = d["pcie_inclusive"]
    assert p["value"] <= d["value"] * 1.02 and len(p["ms_per_step_all"]) == p["repeats"] >= 3


def test_pmc_table_feeds_the_roofline_traffic_fields():
    bench, _ = _bench()
    table, src = bench.pmc_step_traffic("fp32x3")
    assert table is not None and src == "profiles/r06_pmc_traffic_fp32x3.json"
    r = _line()["roofline"]
    per_launch = bench.kernel_traffic(table, r["kernel"])
    # hand computation of the same average: the PMC rows of that kernel (rocprofv3 spells bf16 "unsigned short"), launches-weighted
    tot = n = 0.0
    for k, v in table.items():
        if isinstance(v, dict) and "launches" in v and k.replace("unsigned short", "bf16").replace(" ", "") == r["kernel"].replace(" ", ""):
            tot += (v["fetch_bytes_corrected"] + v["write_bytes"]) * v["launches"]
            n += v["launches"]
    assert n > 0 and per_launch == round(tot / n)
    assert r["traffic_source"] == src and r["traffic"] == per_launch
    assert 0.5e11 < table["_step_total_bytes"] < 3e11 and table["_steps"] >= 1
    assert bench.kernel_traffic(None, r["kernel"]) is None
    # the r01 / r02 label (every plain-A bf16 instantiation of gemm_kernel) still resolves on the bf16 table
    tb, sb = bench.pmc_step_traffic("bf16")
    assert tb is not None and bench.kernel_traffic(tb, "gemm_kernel<bf16,plain>") > 0
    for v in table.values():
        if isinstance(v, dict) and "fetch_bytes_raw" in v:                                   # gfx950 correction of the guide: FETCH_SIZE doubled
            assert abs(v["fetch_bytes_corrected"] - 2.0 * v["fetch_bytes_raw"]) <= 1e-6 * max(1.0, v["fetch_bytes_corrected"])


def test_rocprof_summary_agrees_with_the_live_kernel_timing():
    """The roofline object's launch time comes from HIP events inside bench.py (eager train steps); the committed rocprofv3 --kernel-trace
    --stats summary of the same workload (hipGraph-replayed train steps) must show the same average for that kernel, and for the next ones
    the line lists (tier brief, measurement section)."""
    import re
    r = _line()["roofline"]
    txt = open(os.path.join(ROOT, "profiles", "r06_fp32x3_step_summary.txt")).read()
    avg = {}
    for m in re.finditer(r"n=\s*([0-9.]+)\s+avg=\s*([0-9.]+) us\s+(\S.*)$", txt, re.M):
        avg[m.group(3).replace(" ", "")] = (float(m.group(2)), float(m.group(1)))
    key = r["kernel"].replace(" ", "")
    assert key in avg, f"{r['kernel']} missing from the rocprof summary"
    assert abs(avg[key][0] - r["avg_launch_us"]) < 0.10 * r["avg_launch_us"]
    assert abs(avg[key][1] * 2 - r["launches"]) <= 0.03 * r["launches"]          # 2 instrumented steps (the pillar stem's two internal p3_gemm launches per step are not bracketed by the host timer)
    for nk in r["next_kernels"][:3]:
        k2 = nk["kernel"].replace(" ", "")
        if k2 in avg:
            assert abs(avg[k2][0] - nk["avg_launch_us"]) < 0.15 * nk["avg_launch_us"], nk


def test_bench_gpus_2_launches_two_ranks_itself():
    """`python bench.py --gpus 2` with no launcher around it starts torch.distributed.run as a child (two ranks over gloo here; the step is
    replaced by the dry-run hook because this container has no GPU), relays rank 0's JSON line as the last line of stdout and reports
    n_gpus = 2.  The reference's launch: `torchrun --nproc_per_node=N` (README.md:540) + setup_ddp (misc/shared_utils.py:205-230)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(P3_BENCH_BACKEND="gloo", P3_BENCH_ONE_DEVICE="1", P3_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--lean"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["config"]["collectives"]["world"] == 2 and d["config"]["parallelism"] == "dp2" and d["steps"] == 3
    assert d["config"]["workload"].endswith("x2")


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    import subprocess
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29655", P3_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--lean"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "must agree" in (r.stderr + r.stdout)
