"""bench.py as the driver invokes it -- `python bench.py --gpus N` with no launcher around it -- must start N ranks itself
(R: the reference launches its data-parallel eval under torchrun, groma/eval/eval_rec.py:63-83,122-124).  Exercised here on CPU
with --dry-exchange: the real launcher, torch.distributed.run rendezvous on 127.0.0.1, the gloo process group, bench's own
ShardedJob exchange of the SURVEY-8e row (region logits | pred_boxes | N_i) and the timing contract -- everything but the model."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout  # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_bench_spawns_its_own_ranks_weak():
    r = _run(["--gpus", "2", "--dry-exchange", "--steps", "3", "--warmup", "1", "--batch", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert d["scaling"] == "weak" and d["global_batch"] == 6 and d["shards"] == [3, 3] and d["exchange_ok"]


def test_bench_strong_shards_with_an_empty_rank():
    """global batch 2 over 3 ranks: rank 2 owns no image and still joins every collective"""
    r = _run(["--gpus", "3", "--dry-exchange", "--steps", "2", "--warmup", "1", "--global-batch", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["rccl_ranks"] == 3 and d["scaling"] == "strong" and d["shards"] == [1, 1, 0] and d["exchange_ok"]
    assert d["exchanged_regions"] == 100 + 99   # N_i of global images 0 and 1 as the synthetic rows define them


def test_bench_configs3_verbatim_generate_rows_over_8_ranks():
    """BASELINE configs[3] as the driver would launch it: 8 ranks, greedy generate, global batch 32 = 4 images per GPU.  The row
    carries the P + new_tokens generated ids as f32 (exact below 2^24) + pred_boxes + N_i; per-rank min / max step time is in
    the JSON so load imbalance shows when a node is available."""
    r = _run(["--gpus", "8", "--dry-exchange", "--mode", "generate", "--global-batch", "32", "--batch", "4", "--steps", "2",
              "--warmup", "1"], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["rccl_ranks"] == 8 and d["scaling"] == "strong" and d["shards"] == [4] * 8 and d["global_batch"] == 32
    assert d["mode"] == "generate" and d["row_width"] == 128 + 32 + 400 + 1 and d["exchange_ok"]
    assert 0 < d["ms_per_step_rank_min"] <= d["ms_per_step_rank_max"]


def test_bench_refuses_inconsistent_launches():
    # a launcher exported another world size than --gpus says
    r = _run(["--gpus", "1", "--dry-exchange", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr + r.stdout
    # no GPUs here: the real (non-dry) N-rank launch must fail loudly, not run fewer ranks
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_dist_init_requires_a_launcher():
    import pytest
    from groma_amd import dist as gdist
    old = {k: os.environ.pop(k) for k in ("RANK", "WORLD_SIZE") if k in os.environ}
    try:
        with pytest.raises(RuntimeError):
            gdist.init("gloo")
    finally:
        os.environ.update(old)


def test_host_glue_under_8_way_contention():
    """the forward's host-side glue (GromaModel._host_select: CPU-RNG shuffles + gather lists;
    _host_splice_plan: placeholder splice + scatter rows -- the code propose() / forward() run between the NMS sync and the LLaMA
    launches) timed with 8 ranks competing for this host's cores, 14 images per rank, next to the same code with one rank.
    While no 8-GPU box is available this is the host-side half of multi-GPU readiness: the glue must stay far below the ~150 ms
    a rank's device step takes (the GPU sits idle for exactly this long per step)."""
    one = _json_line(_run(["--gpus", "1", "--dry-exchange", "--host-glue", "--steps", "8", "--warmup", "2", "--batch", "14"]).stdout)
    r = _run(["--gpus", "8", "--dry-exchange", "--host-glue", "--steps", "8", "--warmup", "2", "--batch", "14"], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    g1, g8 = one["host_glue"], d["host_glue"]
    print("host glue us/step: 1 rank", g1, "| 8 ranks", g8)
    assert d["rccl_ranks"] == 8 and g8["images_per_rank"] == 14 and d["exchange_ok"]
    assert 0 < g8["host_glue_us_per_step_rank_min"] <= g8["host_glue_us_per_step_rank_max"]
    assert g8["host_glue_us_per_step_rank_max"] < 20000      # < 20 ms even with 8 python ranks on the 8 cores of this container


def test_full_only_options_are_refused_on_a_plain_run():
    """a plain run measures the headline only; an option that only the legs behind --full can serve fails up front instead of
    quietly writing nothing"""
    assert "--full" in _run(["--help"]).stdout
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0", "--gemm-breakdown", os.devnull])
    assert r.returncode != 0 and "--gemm-breakdown needs --full" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
