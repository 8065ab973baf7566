"""bench.py as the driver runs it at N > 1: ``python bench.py --gpus 2`` starts two ranks (torch.distributed.run child) which,
on this one-GPU box, share the card over gloo - the labelled REHEARSAL of the 8-GPU plumbing.  The JSON line must carry the
driver contract plus the self-checking multi-GPU keys, in the same schema the N = 1 line uses.  GPU only."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")
MULTI = ("collective_world_size", "collective_backend", "self_check", "train_videos_per_s", "train_optimizer_steps_per_s",
         "allreduce_bytes_per_step", "exposed_allreduce_ms_per_step", "exchange")


def _run(argv, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_two_rank_rehearsal_line_is_self_checking():
    d = _run(["--gpus", "2", "--steps", "20", "--min-seconds", "0.5", "--full", "--train-steps", "4", "--no-cpu", "--pixel-steps", "0",
              "--long-video-windows", "0"])
    for k in CONTRACT + MULTI:
        assert k in d, k
    assert d["n_gpus"] == 2 and d["collective_world_size"] == 2 and d["scaling"] == "weak" and d["steps"] == 20
    assert all(d["self_check"].values()), d["self_check"]
    assert "REHEARSAL" in d["collective_backend"] or d["collective_backend"].startswith("rccl")
    assert d["value"] > 0 and d["config"]["finite"] and d["dtype"] == "f32"
    tr = d["train"]
    assert tr["global_batch"] == 4 and tr["allreduce_bytes_per_step"] == 4 * tr["params"] == d["allreduce_bytes_per_step"]
    ex = tr["exchange"]
    assert ex["world_size"] == 2 and sum(ex["bucket_bytes"]) == tr["allreduce_bytes_per_step"] and len(ex["bucket_bytes"]) >= 2
    assert ex["buckets_started_inside_the_backward"] + ex["buckets_started_after_the_backward"] == len(ex["bucket_bytes"]) * (4 + 4)
    assert d["exchange"]["bucket_bytes"] == ex["bucket_bytes"]
    assert tr["roofline"]["flops_per_step"] > 2.5e11 and 0 < tr["roofline"]["frac"] < 1
    assert tr["last_loss"] == tr["last_loss"]          # not NaN


def test_one_rank_line_has_the_same_schema():
    d = _run(["--steps", "50", "--min-seconds", "0.5", "--full", "--train-steps", "6", "--machinery-steps", "6", "--no-cpu",
              "--pixel-steps", "0", "--long-video-windows", "0", "--no-breakdown"])
    for k in CONTRACT + MULTI:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["collective_world_size"] == 1 and d["allreduce_bytes_per_step"] == 0
    assert d["exposed_allreduce_ms_per_step"] == 0.0 and all(d["self_check"].values())
    assert d["per_chain_setup"]["fallback"] is None and d["per_chain_setup"]["timestep_table_bytes"] > 0
    # the headline through the public API: one whole 1000-step chain of diffusion.p_sample_loop
    assert d["p_sample_loop_wall_ms"] > 0 and d["steps_per_s_public_api"] > 0 and d["public_api"]["finite"]
    assert abs(d["steps_per_s_public_api"] / d["value"] - 1.0) < 0.06, (d["steps_per_s_public_api"], d["value"])   # (50-step regions are noisy)
    # what one GPU can report about the exchange with today's code: the machinery forced on at world size 1 (RCCL)
    ex = d["train"]["exchange"]
    assert isinstance(ex["machinery_ms_per_step"], float) and -1.0 < ex["machinery_ms_per_step"] < 5.0, ex
    assert ex["overlap_probe"] is not None and "ok" in ex["overlap_probe"], ex
    assert ex["machinery"]["buckets"] >= 2 and ex["machinery"]["backend"] == "nccl"
    assert ex["machinery"]["buckets_started_inside_the_backward"] > 0 or not ex["overlap_probe"]["ok"]
    assert d["exchange"]["machinery_ms_per_step"] == ex["machinery_ms_per_step"] and d["exchange"]["overlap_probe"] == ex["overlap_probe"]
    # memory-bound phases against the HBM peak
    hp = d["hbm_phases"]
    for k in ("adamw_ema", "q_sample", "masked_mse"):
        assert hp[k]["bytes"] > 0 and hp[k]["us"] > 0 and 0 < hp[k]["frac"] < 1, (k, hp[k])
    assert hp["adamw_ema"]["frac"] > 0.4, hp["adamw_ema"]
    assert d["code_stamp"]["abi"] > 0


def test_plain_line_times_exactly_its_steps_and_dumps_the_last_one(tmp_path):
    """Without --full: one timed region of exactly --steps steps, the headline keys and none of the extra legs; with
    --dump-outputs the sample and pred_xstart after the last timed step, the same in two runs with the same arguments."""
    import numpy as np
    dumps = []
    for run in range(2):
        out_dir = tmp_path / f"run{run}"
        d = _run(["--steps", "24", "--warmup", "5", "--dump-outputs", str(out_dir)])
        for k in CONTRACT:
            assert k in d, k
        assert d["steps"] == 24 and d["warmup"] == 5 and d["timed_regions"] == 1 and d["n_gpus"] == 1
        assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1000.0 - 1.0) < 1e-3, d
        for k in ("public_api", "train", "long_video", "pixel", "roofline", "breakdown", "hbm_phases", "cpu_baseline"):
            assert k not in d, k
        arrays = {n: np.load(out_dir / f"{n}.npy") for n in ("sample", "pred_xstart")}
        for n, a in arrays.items():
            assert a.dtype == np.float32 and a.shape == (2, 20, 4, 16, 16) and np.isfinite(a).all(), n
        dumps.append(arrays)
    # (launch tuning may pick another tile shape in the second run; x0-hat divides by sqrt(alpha_bar) ~ 0.01 near t = 999)
    np.testing.assert_allclose(dumps[1]["sample"], dumps[0]["sample"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dumps[1]["pred_xstart"], dumps[0]["pred_xstart"], rtol=1e-4, atol=1e-3)


def test_pixel_training_leg_runs_the_published_recipe():
    """bench.bench_pixel_train: the reference's published training recipe (README.md:54-57: 128x128x3 frames, 20 frames,
    num_channels=128, num_res_blocks=1) as a TrainLoop at batch 1 - eager steps, capture, replays; finite loss, a captured
    micro-step, and a whole-step rate that only the large-map kernels (chunked GroupNorm backward, tiled weight gradients)
    can give: above 40 % of the fp32 MFMA peak."""
    import sys
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.setdefault("LFVDM_TUNE_CACHE", os.path.join(ROOT, "profiles", "tune_cache_mi355x.json"))
    import bench
    rec = bench.bench_pixel_train(torch.device("cuda", 0), 3, batch=1, num_res_blocks=1, warmup=4)
    assert rec["graph_replay"] and rec["last_loss"] == rec["last_loss"] and 0.0 < rec["last_loss"] < 10.0, rec
    assert rec["params"] == 80358147
    rf = rec["roofline"]
    assert rf["flops_per_step"] > 5.0e12 and rf["frac"] > 0.40, rf
    fam = rf.get("families")
    if fam is not None and not fam["stale"]:
        assert fam["slowest_groupnorm_kernel_avg_us"] < 100.0, fam
