"""bench.py as its own multi-rank launcher (VERDICT r1 "Next round" item 1).

`python bench.py --gpus N` with no WORLD_SIZE must start N rank processes itself, relay ONE
JSON line whose n_gpus / world_size_seen are N, fail loudly when a rank fails, and never run
fewer ranks than asked. Driven here with --device cpu (gloo, CPU tensors): the launcher,
rendezvous, timing brackets, rank-max reduction and JSON assembly are the same code the GPU
run uses.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BENCH = str(ROOT / "bench.py")


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, env=env)


@pytest.mark.parametrize("n,negatives", [(2, "symmetric"), (3, "allgather")])
def test_launcher_spawns_ranks_and_relays_one_json_line(n, negatives):
    r = _run(["--device", "cpu", "--gpus", str(n), "--batch", "16", "--dim", "8", "--steps", "3", "--warmup", "1",
              "--dtype", "fp32", "--negatives", negatives, "--full"])  # --full: the communication-wait pass
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["world_size_seen"] == n
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["config"]["global_batch"] == n * 16 and d["config"]["parallelism"] == f"dp{n}"
    assert d["value"] == pytest.approx(n * 16 / (d["ms_per_step"] / 1e3), rel=1e-3)
    assert len(d["comm_wait_ms_per_step_per_rank"]) == n
    assert d["loss"] == d["loss"]  # finite
    # host cost of the multi-rank step (verdict r5: the N > 1 step must be shown GPU-bound)
    he = d["host_enqueue_ms_per_step"]
    assert isinstance(he, float) and math.isfinite(he) and he > 0.0, he
    assert d["config"]["dist_impl"] in (None, "engine", "torch")


def test_rank_failure_fails_the_job():
    r = _run(["--device", "cpu", "--gpus", "2", "--batch", "8", "--dim", "8", "--steps", "2", "--warmup", "1",
              "--dtype", "fp32", "--timeout", "120"], {"NTXENT_BENCH_FAIL_RANK": "1"})
    assert r.returncode != 0
    assert "rank 1 exited with code 3" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_world_size_mismatch_is_an_error():
    r = _run(["--device", "cpu", "--gpus", "8", "--batch", "8", "--dim", "8"], {"WORLD_SIZE": "1"})
    assert r.returncode != 0 and "--gpus 8" in r.stderr


def test_single_rank_cpu_json_contract():
    r = _run(["--device", "cpu", "--batch", "16", "--dim", "8", "--steps", "2", "--warmup", "1", "--dtype", "fp32"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["metric"] == json.loads((ROOT / "BASELINE.json").read_text())["metric"]
    # host CPU time to issue one step (verdict r3: the wall-vs-event gap), measured in the timed run
    assert 0.0 < d["host_enqueue_ms_per_step"] and d["host_enqueue_note"]
    assert d["value"] == pytest.approx(16 / (d["ms_per_step"] / 1e3), rel=1e-3)


def _load_dump(d):
    import numpy as np

    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_plain_run_and_dump_outputs_cpu(tmp_path):
    """A run without --full skips the extra passes (their fields are null), --steps is the number of
    timed steps, and --dump-outputs writes the last timed step's loss and gradient as float32
    arrays that a second run with the same arguments reproduces exactly."""
    import numpy as np

    args = ["--device", "cpu", "--gpus", "2", "--batch", "16", "--dim", "8", "--steps", "3", "--warmup", "1",
            "--dtype", "fp32"]
    docs, dumps = [], []
    for i in range(2):
        r = _run([*args, "--dump-outputs", str(tmp_path / f"d{i}")])
        assert r.returncode == 0, r.stderr[-2000:]
        docs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        dumps.append(_load_dump(tmp_path / f"d{i}"))
    d = docs[0]
    assert d["full"] is False and d["steps"] == 3 and d["ms_per_step"] > 0.0
    assert d["comm_wait_ms_per_step"] is None and d["comm_wait_ms_per_step_per_rank"] is None
    assert d["step_ms"] is None and d["secondary"] is None
    a, b = dumps
    assert sorted(a) == ["grad", "loss"] and sorted(b) == ["grad", "loss"]
    assert a["grad"].dtype == np.float32 and a["loss"].dtype == np.float32
    assert a["grad"].shape == (32, 8) and a["loss"].shape == ()
    assert np.isfinite(a["grad"]).all() and np.abs(a["grad"]).max() > 0.0
    assert float(a["loss"]) == pytest.approx(d["loss"], rel=1e-6)
    assert np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["loss"], b["loss"])


def test_dump_outputs_samples_large_gradients(tmp_path):
    """Above DUMP_MAX_BYTES the gradient is cut to a fixed row sample: same rows on every call,
    ascending, within the size limit."""
    import numpy as np
    import torch

    sys.path.insert(0, str(ROOT))
    import bench

    rows, dim = 4096, 4096  # 64 MiB as float32
    gh = torch.arange(rows, dtype=torch.float32)[:, None].expand(rows, dim)
    got = []
    for i in range(2):
        bench.dump_outputs(str(tmp_path / f"s{i}"), torch.tensor(1.5), gh)
        got.append(_load_dump(tmp_path / f"s{i}"))
    g = got[0]["grad"]
    keep = bench.DUMP_MAX_BYTES // (4 * dim)
    assert g.shape == (keep, dim) and g.dtype == np.float32 and g.nbytes <= bench.DUMP_MAX_BYTES
    assert (np.diff(g[:, 0]) > 0).all() and (g == g[:, :1]).all()  # whole rows, ascending, distinct
    assert np.array_equal(g, got[1]["grad"]) and float(got[0]["loss"]) == 1.5


@pytest.mark.gpu
def test_plain_gpu_run_dumps_last_step(tmp_path):
    """The headline shape on the GPU, plain: no extra passes, and the dumped loss / gradient sample
    are those of the last timed step (float32, finite, within the dump's size limit)."""
    import numpy as np

    sys.path.insert(0, str(ROOT))
    import bench

    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--prewarm-steps", "2", "--dump-outputs",
              str(tmp_path / "d")])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["full"] is False and d["steps"] == 2 and d["step_ms"] is None and d["secondary"] is None
    assert d["dtype"] == "bf16" and d["value"] == pytest.approx(4096 / (d["ms_per_step"] / 1e3), rel=1e-3)
    got = _load_dump(tmp_path / "d")
    assert sorted(got) == ["grad", "loss"]
    g = got["grad"]
    assert g.dtype == np.float32 and g.shape == (bench.DUMP_MAX_BYTES // (4 * 2048), 2048)
    assert sum(v.nbytes for v in got.values()) <= 64 * 10**6
    assert np.isfinite(g).all() and (np.abs(g).max(axis=1) > 0.0).all()  # every sampled row was written
    assert got["loss"].dtype == np.float32 and float(got["loss"]) == pytest.approx(d["loss"], rel=1e-6)


def test_scaling_driver_cpu():
    """bench/scaling.py: runs bench.py per N and reports both efficiencies."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench" / "scaling.py"), "--ns", "1,2", "--device", "cpu",
                        "--batch", "16", "--dim", "8", "--steps", "2", "--warmup", "1", "--dtype", "fp32",
                        "--timeout", "120"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    assert [c["n_gpus"] for c in doc["curve"]] == [1, 2]
    c1, c2 = doc["curve"]
    assert c1["samples_efficiency"] == pytest.approx(1.0) and c1["pair_efficiency"] == pytest.approx(1.0)
    assert c2["pair_efficiency"] == pytest.approx(2 * c2["samples_efficiency"], rel=1e-3)  # JSON rounding
    assert doc["runs"]["2"]["n_gpus"] == 2


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_rank_env_maps_rank_r_to_cuda_r(n):
    """The driver's scaling run at N = 8: the launcher gives rank r LOCAL_RANK r (and the
    torchrun-style variables), and a rank places itself on cuda:LOCAL_RANK — one rank per GPU,
    every GPU used once; the one-GPU rehearsal (--share-gpu) puts every rank on cuda:0. The
    process group is initialised with device_id = that device (bench.py run_rank)."""
    sys.path.insert(0, str(ROOT))
    import bench

    envs = [bench.rank_env({"PATH": "/bin"}, r, n, 29500) for r in range(n)]
    assert [e["RANK"] for e in envs] == [str(r) for r in range(n)]
    assert [e["LOCAL_RANK"] for e in envs] == [str(r) for r in range(n)]
    assert all(e["WORLD_SIZE"] == str(n) and e["LOCAL_WORLD_SIZE"] == str(n) for e in envs)
    assert all(e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29500" for e in envs)
    assert all(e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and e[bench.CHILD_ENV] == "1" for e in envs)
    devs = [bench.rank_device(int(e["LOCAL_RANK"]), share_gpu=False) for e in envs]
    assert devs == list(range(n))
    assert {bench.rank_device(int(e["LOCAL_RANK"]), share_gpu=True) for e in envs} == {0}
    # the GPU rank path initialises RCCL with the rank's own device (no implicit device 0)
    src = (ROOT / "bench.py").read_text()
    assert 'dist.init_process_group("nccl", device_id=dev' in src
    assert "dev_index = rank_device(local_rank, a.share_gpu)" in src


def test_w8_full_check_plumbing_on_cpu(tmp_path):
    """tools/w8_full_check.py (the config-3-size rehearsal the GPU box runs at W = 8, B = 4096/rank,
    d = 2048) on CPU tensors over gloo: symmetric vs all-gather vs the fp32 torch oracle, and the
    one-line JSON it writes."""
    out = tmp_path / "w.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
                        "--master-addr", "127.0.0.1", "--master-port", "29781",
                        str(ROOT / "tools" / "w8_full_check.py"), "--device", "cpu", "--batch", "300", "--dim", "48",
                        "--json-out", str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(out.read_text())
    assert d["ok"] and d["world"] == 3 and len(d["per_rank"]) == 3
    assert abs(d["loss_symmetric"] - d["loss_fp32_torch"]) <= 1e-5 * abs(d["loss_fp32_torch"])
