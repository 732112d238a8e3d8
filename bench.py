#!/usr/bin/env python
"""bench.py -- headline metric of BASELINE.json on MI355X:
images/sec of the end-to-end Groma forward (448 px, 300 proposals -> 100 regions, 128-token prompt, logits for all
582 positions as the reference computes them), DINOv2-L + DDETR + region encoder + Vicuna-7B, random-init weights; 16-bit operands (HEADLINE_DTYPE below).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one forward pass of the hot path over one per-GPU batch of synthetic images already resident in HBM.
Multi-GPU: image batch sharded across ranks (weak scaling, full replica per GPU), one RCCL all-gather of the
per-image region logits per step.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def flops_per_image(cfg, N, P):
    """Algorithmic FLOPs of one image's forward (2MNK per GEMM/conv, 4*T^2*d per attention layer)."""
    vc, dc, lc, rc = cfg.perceiver_cfg.vis_encoder_cfg, cfg.perceiver_cfg.ddetr_cfg, cfg.llm_cfg, cfg.region_cfg
    D, g = vc.hidden_size, cfg.image_size // vc.patch_size
    T = g * g + 1
    vit = 2 * g * g * D * 3 * vc.patch_size ** 2 + vc.num_hidden_layers * (2 * T * D * D * (4 + 2 * vc.mlp_ratio) + 4 * T * T * D)
    Tt = lc.hidden_size
    bridge = 2 * (g // 2) ** 2 * (4 * D * Tt + Tt * Tt)
    d, HW, Q, F = dc.d_model, g * g, dc.two_stage_num_proposals, dc.encoder_ffn_dim
    enc = dc.encoder_layers * 2 * HW * (d * d * 2 + d * 96 + 2 * d * F)
    dec = dc.decoder_layers * (2 * Q * (d * d * 4 + d * 96 + d * d + 2 * d * F) + 2 * HW * d * d + 4 * Q * Q * d)
    ddetr = 2 * HW * D * d + enc + dec + 2 * HW * d * d * 3 + 2 * Q * (2 * d) ** 2
    pos = sum((g * 2 ** l) ** 2 for l in range(3))
    region = 2 * pos * (D + 2) * D + rc.num_fuse * 2 * pos * 9 * D * D
    P2 = rc.roi_size ** 2
    region += N * (3 * 2 * P2 * 9 * D * D + 2 * P2 * D * rc.mid_dim + 2 * rc.mid_dim * Tt)
    L = P - 2 + (g // 2) ** 2 + 2 * N
    per_layer = 2 * Tt * (4 * Tt + 3 * lc.intermediate_size)
    V = lc.vocab_size + cfg.num_new_token
    llm = lc.num_hidden_layers * (L * per_layer + 4 * L * L * Tt) + 2 * L * Tt * V
    return dict(vit=vit, bridge=bridge, ddetr=ddetr, region=region, llm=llm, total=vit + bridge + ddetr + region + llm, L=L)


class _AliasedLayers(dict):
    """state dict whose per-layer entries of the three deep stacks all resolve to layer 0: a FULL-DEPTH oracle forward then
    needs one materialised layer per stack (3 GB instead of 30 GB of host RAM, seconds instead of minutes of randn) while
    executing every layer's arithmetic and memory traffic -- the weights of a 0.8 GB layer never stay in cache anyway."""
    import re as _re
    _pat = _re.compile(r"(vis_encoder\.encoder\.layer|mlvl_fuse\.fuse_convs|llm\.model\.layers)\.\d+\.")

    def _k(self, k):
        return self._pat.sub(lambda m: m.group(1) + ".0.", k)

    def __getitem__(self, k):
        return dict.__getitem__(self, self._k(k))

    def get(self, k, default=None):
        return dict.get(self, self._k(k), default)

    def __contains__(self, k):
        return dict.__contains__(self, self._k(k))


def cpu_baseline(cfg_name, threads=None, full_reps=1):
    """The oracle (plain PyTorch fp32 restatement, oracle/groma_oracle.py) on this box's host cores, ONE image.
      value  = a MEASURED full-depth forward (24 ViT layers, 6+6 DDETR, NMS, 5 fusion rounds, RoI extraction, 32 LLaMA
               layers, 32 114-wide head over all 582 positions), median of `full_reps` runs (default 1: ~40 s of CPU work;
               the reduced-depth pass just before it is the warm-up).  Layer weights of the three deep stacks are aliased
               to one materialised layer each (_AliasedLayers) -- same arithmetic, bounded host RAM.
      sample = also carries the round-1 style extrapolation (reduced depth x layer counts) for comparison."""
    from groma_amd import config as gconfig, synth
    from oracle import groma_oracle as O
    if threads:
        torch.set_num_threads(threads)
    full = gconfig.groma_7b(box_score_thres=0.0) if cfg_name == "7b" else gconfig.groma_tiny(box_score_thres=0.0)
    nv, nf, nl = full.perceiver_cfg.vis_encoder_cfg.num_hidden_layers, full.region_cfg.num_fuse, full.llm_cfg.num_hidden_layers
    d = full.to_dict()
    d.pop("vocab_size")
    d["perceiver_cfg"]["vis_encoder_cfg"]["num_hidden_layers"] = 1
    d["region_cfg"]["num_fuse"] = 1
    d["llm_cfg"]["num_hidden_layers"] = 1
    small = gconfig.GromaConfig(**d)
    sd = _AliasedLayers(synth.make_state_dict(small, 0))
    cd = small.to_dict()
    from tests.util import TokenIds, tok_dict
    tk = TokenIds()
    images, ids = synth.make_inputs(small, tk, 1, seed=1234)

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    with torch.no_grad():
        # reduced depth (one layer of each deep stack), per-stage -> extrapolation + warm-up of the thread pool
        O.vit_forward(sd, cd, images)
        t_vit, hs4 = timed(lambda: O.vit_forward(sd, cd, images))
        cd2 = full.to_dict()
        cd2["perceiver_cfg"]["vis_encoder_cfg"]["num_hidden_layers"] = 3  # 4 states for the proposer (aliased weights)
        hs = O.vit_forward(sd, cd2, images)
        t_det, det = timed(lambda: O.ddetr_forward(sd, cd, O.ddetr_inputs_from_hidden(hs)))
        scores = O.fuse_scores(det["logits_coco"], det["logits_sa1b"])
        torch.manual_seed(0)
        sel, _, _ = O.select_regions(det["pred_boxes"], scores, None, None, 0.6, 0.0, 100)
        mlvl = [h[:, 1:] for h in hs[-3:]]
        t_fuse, feats = timed(lambda: O.region_fuse(sd, cd, mlvl))
        t_roi, reg = timed(lambda: O.roi_extract(sd, cd, feats, sel))
        L = ids.shape[1] - 2 + 256 + 2 * len(sel[0])
        emb = torch.randn((1, L, small.llm_cfg.hidden_size)) * 0.02
        t_llm, (hid, _) = timed(lambda: O.llama_forward(sd, cd, emb, torch.ones((1, L))))
        t_head, _ = timed(lambda: O.lm_logits(sd, hid))
        extrap = t_vit * nv + t_det + t_fuse * nf + t_roi + t_llm * nl + t_head
        # the measurement: a full-depth forward through the oracle's own entry point
        fd = full.to_dict()
        runs = []
        for _ in range(max(1, full_reps)):
            torch.manual_seed(0)
            t, ref = timed(lambda: O.groma_forward(sd, fd, tok_dict(tk), ids.clone(), images))
            runs.append(t)
        runs.sort()
        t_full = runs[len(runs) // 2]
        assert ref["logits"].shape[1] == L
    return {"value": 1.0 / t_full, "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "seconds_per_image": t_full,
            "sample": f"1 image, MEASURED full-depth fp32 oracle forward ({nv} ViT layers, {full.perceiver_cfg.ddetr_cfg.encoder_layers}+{full.perceiver_cfg.ddetr_cfg.decoder_layers} DDETR, NMS, {nf} fusion rounds, "
                      f"{len(sel[0])} regions, {nl} LLaMA layers, logits for all {L} positions), median of {len(runs)} run(s) "
                      f"after a reduced-depth warm-up; per-layer weights of the deep stacks aliased to one layer each. "
                      f"For comparison, reduced-depth extrapolation: {extrap:.1f} s/image "
                      f"(vit {t_vit * nv:.2f}, ddetr {t_det:.2f}, region {t_fuse * nf + t_roi:.2f}, llm {t_llm * nl + t_head:.2f})"}


def measure_traffic(batch, kernel="gemm_bf16_256_kernel", extra=()):
    """HBM-side traffic of the dominant kernel, measured NOW: two separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE --
    they do not fit one pass on gfx950) of `bench.py --steps 1 --warmup 1 --batch B` as child processes, exactly the recipe of
    MI355X_MICROARCH.md (cwd /tmp, TMPDIR=/tmp, counters with --kernel-trace only).  Returns bytes per launch with the guide's
    gfx950 correction (FETCH_SIZE counts a wide streaming read at half its bytes -> x2), or None if the profiler is unavailable."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    tmp = tempfile.mkdtemp(prefix="groma_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    avg = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = ["rocprofv3", "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable,
                   os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--batch", str(batch), "--no-cpu-baseline",
                   "--no-traffic", "--no-extras", "--no-prefill-graphs"] + list(extra)   # (eager launches: no graph set-up passes under the profiler)
            # own process group: on a timeout the profiler AND the python under it are ended (exactly the group started here), so a hung
            # pass can neither outlive this call nor keep the GPU busy under the timed steps that follow
            proc = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = proc.wait(timeout=150)   # (normally ~25 s)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(proc.pid, signal.SIGKILL)
                proc.wait()
                return None
            if rc != 0:
                return None
            tot, n = 0.0, 0
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r["Counter_Name"] == ctr and kernel in r["Kernel_Name"]:   # (a template since round 4: "void gemm_bf16_256_kernel<8>(GemmArgs)")
                        tot += float(r["Counter_Value"])
                        n += 1
            if n == 0:
                return None
            avg[ctr] = tot / n
        return (2.0 * avg["FETCH_SIZE"] + avg["WRITE_SIZE"]) * 1024.0
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def launch_ranks(args, argv):
    """`python bench.py --gpus N` with no launcher around it: become the launcher.  Re-executes this file under
    torch.distributed.run with one process per GPU (the reference launches its data-parallel eval the same way:
    groma/eval/eval_rec.py:63-83 under torchrun), rendezvous on 127.0.0.1, and returns the children's exit code.  Refuses
    (non-zero) when fewer than N devices are visible instead of quietly measuring fewer ranks."""
    import subprocess
    if not args.dry_exchange:
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but only {n_dev} GPU(s) visible", file=sys.stderr)
            return 3
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL across processes needs it on this driver)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    return subprocess.run(cmd, env=env).returncode


ROW_BOXES = 400  # 100 region slots x (cx, cy, w, h)


def pack_rows(head, boxes_list):
    """One f32 row per image for the step's single all-gather: [head | 100 x 4 box slots (zero padded) | N_i].
    head = the <r0..r99> logits of the last position (forward) or the generated ids (generate; ids < 2^24 are exact in f32)."""
    b = head.shape[0]
    out = torch.zeros((b, head.shape[1] + ROW_BOXES + 1), dtype=torch.float32, device=head.device)
    out[:, : head.shape[1]] = head
    if boxes_list and all(x.shape[0] == boxes_list[0].shape[0] for x in boxes_list):   # the benchmark: N_i = 100 everywhere
        n = boxes_list[0].shape[0]
        out[:, head.shape[1]: head.shape[1] + 4 * n] = torch.stack(boxes_list).reshape(b, 4 * n)
        out[:, -1] = float(n)
    else:
        for i, bx in enumerate(boxes_list):
            out[i, head.shape[1]: head.shape[1] + 4 * bx.shape[0]] = bx.reshape(-1)
            out[i, -1] = float(bx.shape[0])
    return out


def run_dry_exchange(args, rank, world):
    """No model, no GPU: the launcher + process group + ShardedJob exchange + timing contract with synthetic rows (gloo).
    What tests/test_bench_launcher.py runs with 2 ranks on CPU."""
    from groma_amd import dist as gdist
    dev = torch.device("cpu")
    if world > 1:
        gdist.init("gloo", None)
    strong = args.global_batch > 0
    gen = args.mode == "generate"
    # the row head is what the real step packs: 100 region logits, or -- configs[3], --mode generate -- the P + new_tokens ids of
    # `sequences` carried as f32 (token ids < 2^24 are exact in f32; the dry run checks the round trip)
    head = (128 + args.new_tokens) if gen else 100
    job = gdist.ShardedJob(dev, (head + ROW_BOXES + 1,), torch.float32,
                           **(dict(global_batch=args.global_batch) if strong else dict(rows_per_rank=args.batch)))
    ranks = gdist.count_ranks(dev)

    def rows_of(lo, hi, i):   # deterministic function of the GLOBAL image index, so rank 0 can check what it gathered
        idx = torch.arange(lo, hi, dtype=torch.float32)
        if gen:   # synthetic token ids over the whole 32 114-entry vocabulary, as int64 -> f32 like pack_rows(g.sequences.float(), ...)
            ids = (idx.long()[:, None] * 7919 + torch.arange(head)[None] * 104729 + i) % 32114
            heads = ids.float()
            assert torch.equal(heads.long(), ids)
        else:
            heads = idx[:, None] * 1000.0 + torch.arange(head, dtype=torch.float32)[None] + float(i)
        boxes = [torch.full((100 - (int(g) % 3), 4), float(g)) for g in idx]
        return pack_rows(heads, boxes)

    last = {}
    # --host-glue: every rank also runs, per step, the REAL host code a forward executes between the NMS result and the LLaMA
    # launches (GromaModel._host_select: CPU-RNG shuffles + gather lists; _host_splice_plan: placeholder splice, scatter rows) for its
    # share of the batch -- no model weights, no device -- so `host_glue_us_per_step` is that code's cost under N-way contention
    # for the host cores (multi-GPU readiness needs a host-side number while no 8-GPU box is available)
    glue_us = []
    if args.host_glue:
        import time as _time
        from groma_amd import config as gconfig, constants
        from groma_amd.groma import GromaModel
        gm = GromaModel(gconfig.groma_7b(box_score_thres=0.0))
        gm.init_special_token_id(constants.SyntheticTokenizer())
        from groma_amd import synth
        _, prompt_ids = synth.make_inputs(gconfig.groma_tiny(), gm, max(job.rows, 1), seed=7, prompt_len=128)
        keep_h = torch.stack([torch.randperm(300)[:100] for _ in range(max(job.rows, 1))])

        def host_glue():
            t0 = _time.perf_counter()
            sel_idx, flat_sel, img_of = GromaModel._host_select(keep_h, [100] * keep_h.shape[0], 300)
            plan = gm._host_splice_plan(prompt_ids.clone(), 256, [int(x.numel()) for x in sel_idx])
            glue_us.append((_time.perf_counter() - t0) * 1e6)
            return plan

    def step(i):
        if args.host_glue and job.rows:
            host_glue()
        last["i"], last["out"] = i, job.exchange(rows_of(job.lo, job.hi, i)) if job.rows else job.exchange(torch.zeros((0, head + ROW_BOXES + 1)))
        return last["out"]
    elapsed = job.timed(step, args.warmup, args.steps)
    glue = None
    if args.host_glue:   # median over this rank's timed steps, then max / min over ranks
        mine = sorted(glue_us[-args.steps:])[len(glue_us[-args.steps:]) // 2] if glue_us else 0.0
        t = torch.tensor([mine], dtype=torch.float64)
        hi, lo = t.clone(), t.clone()
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        glue = {"host_glue_us_per_step_rank_max": float(hi), "host_glue_us_per_step_rank_min": float(lo), "images_per_rank": job.rows,
                "host_threads_per_rank": torch.get_num_threads(), "host_cores": os.cpu_count()}
    ok = torch.equal(last["out"], rows_of(0, job.global_batch, last["i"]))
    if rank == 0:
        print(json.dumps({"metric": "dry exchange (no model)", "value": job.global_batch * args.steps / elapsed, "unit": "rows/s",
                          "n_gpus": world, "rccl_ranks": ranks, "backend": "gloo", "steps": args.steps, "warmup": args.warmup,
                          "scaling": "strong" if strong else "weak", "global_batch": job.global_batch, "shards": job.counts,
                          "mode": args.mode, "row_width": head + ROW_BOXES + 1,
                          "ms_per_step_rank_max": job.last_elapsed_max / max(args.steps, 1) * 1e3,
                          "ms_per_step_rank_min": job.last_elapsed_min / max(args.steps, 1) * 1e3,
                          "exchange_ok": bool(ok), "exchanged_regions": int(last["out"][:, -1].sum().item()),
                          **({"host_glue": glue} if glue else {})}), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0 if ok else 1


def measure(model, cfg, args, dev, rank, job, P, gen, batch, plan="throughput", steps=None, warmup=None, strong=False, keep=None):
    """time `steps` steps of the hot path at `batch` images per forward call through `job`; returns (seconds, step_fn).
    job.last_rows: the exchanged rows of the LAST timed step (valid until the next step).
    keep: a dict that receives, as host arrays, what the LAST timed step handed its caller (see dump_arrays)"""
    from groma_amd import synth
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    if strong:   # the same global images whatever the world size; this rank keeps its shard
        images, ids = synth.make_inputs(cfg, model, job.global_batch, seed=1234, prompt_len=P)
        images, ids = images[job.lo:job.hi], ids[job.lo:job.hi]
    else:
        images, ids = synth.make_inputs(cfg, model, job.rows, seed=1234 + rank, prompt_len=P)
    images, ids = images.to(dev), ids.to(dev)
    r0 = model.box_idx_token_ids[0]
    chunks = [(lo, min(lo + batch, job.rows)) for lo in range(0, job.rows, batch)]
    width = job.row_shape[0]

    last_timed = warmup + steps - 1
    held = {}   # device tensors of the last timed step (references only: copied to the host after the timed region)

    def step(i):
        torch.manual_seed(1000 + i)  # the path draws torch.randperm (T4)
        hold = keep is not None and i == last_timed
        rows = []
        for lo, hi in chunks:
            if gen:
                g = model.generate(ids[lo:hi], images=images[lo:hi], max_new_tokens=args.new_tokens, return_dict_in_generate=True,
                                   output_hidden_states=True)
                rows.append(pack_rows(g.sequences.float(), g.hidden_states[0][-1]["pred_boxes"]))
                if hold:
                    held.setdefault("sequences", []).append(g.sequences)
                    held.setdefault("pred_boxes", []).extend(g.hidden_states[0][-1]["pred_boxes"])
            else:
                out = model.forward(input_ids=ids[lo:hi], images=images[lo:hi], use_cache=False, return_dict=True)
                rows.append(pack_rows(out.logits[:, -1, r0:r0 + 100], out.hidden_states[1]["pred_boxes"]))
                if hold:
                    held.setdefault("logits", []).append(out.logits)
                    held.setdefault("pred_boxes", []).extend(out.hidden_states[1]["pred_boxes"])
        if not rows:   # a rank whose shard is empty (global batch < world): it still takes part in the collective
            res = job.exchange(torch.zeros((0, width), dtype=torch.float32, device=dev))
        else:
            res = job.exchange(rows[0] if len(rows) == 1 else torch.cat(rows))
        if i == last_timed:
            held["rows"] = res
        return res

    old = model.gemm_plan
    model.gemm_plan = plan
    caps = lambda: model.vit.graphs.captures + model.llm.graphs.captures + model.region.graphs.captures
    mark = {}
    try:
        # hipGraph capture is set-up, like building the model: a shape is captured on its third sighting (GraphPool.CAPTURE_AT), so
        # with fewer than that many warm-up steps the missing sightings are run here, before the W untimed + K timed steps
        from groma_amd import engine
        job.setup_steps = max(0, engine.GraphPool.CAPTURE_AT - warmup) if engine.GraphPool.enabled else 0
        for i in range(job.setup_steps):
            step(-1 - i)
        elapsed = job.timed(step, warmup, steps, after_warmup=lambda: mark.update(c=caps()))
        # what the exchange delivered at the last timed step; read before any further step: graph replays reuse their output buffers
        job.last_rows = held.get("rows")
        if keep is not None:
            keep.update(dump_arrays(held))
        held.clear()
    finally:
        model.gemm_plan = old
    # a hipGraph capture (GraphPool: third sighting of a shape) inside the timed region would put a capture pass and a
    # stream sync into the measurement: counted, reported, and 0 whenever warmup >= GraphPool.CAPTURE_AT
    job.captures_in_timed_region = caps() - mark.get("c", caps())
    return elapsed, step


DUMP_LOGITS_SAMPLE = 1 << 21   # logits elements kept per dump (all images together): 8 MB of float32
DUMP_LAST_ROWS = 128            # images whose last-position logits are kept whole (128 x 32114 x 4 B = 16 MB)


def dump_arrays(held):
    """Host float32 / float64 copies of what one step handed its caller, at most ~36 MB whatever the batch:
      rows           [global_batch, head + 401]  the step's exchanged rows (region logits or generated ids | boxes | N_i)
      pred_boxes     [images, max N_i, 4]        the selected boxes of every image, zero padded; n_regions [images] holds N_i
      logits_last    [min(images, 128), V]       forward: the last position's logits, whole
      logits_sample  [images, k]                 forward: the logits at k fixed flat positions of every image's [L, V] block,
      logits_sample_index [k]                    listed (float64) in logits_sample_index; drawn by numpy's default_rng(0)
      sequences      [images, P + new tokens]    generate: the token ids (float64, exact)"""
    import numpy as np
    out = {"rows": held["rows"].float().cpu().numpy()}
    boxes = held.get("pred_boxes", [])
    n = [int(b.shape[0]) for b in boxes]
    pb = np.zeros((len(boxes), max(n, default=0), 4), dtype=np.float32)
    for i, b in enumerate(boxes):
        pb[i, : n[i]] = b.float().cpu().numpy().reshape(-1, 4)
    out["pred_boxes"], out["n_regions"] = pb, np.asarray(n, dtype=np.float32)
    if "logits" in held:
        lg = held["logits"]
        images = sum(x.shape[0] for x in lg)
        block = min(x.shape[1] * x.shape[2] for x in lg)   # (every image of the benchmark has the same [L, V]; else the common prefix)
        k = min(block, max(1, DUMP_LOGITS_SAMPLE // max(images, 1)))
        idx = np.sort(np.random.default_rng(0).choice(block, size=k, replace=False))
        t_idx = torch.from_numpy(idx).to(lg[0].device)
        out["logits_sample"] = torch.cat([x.reshape(x.shape[0], -1)[:, t_idx].float() for x in lg]).cpu().numpy()
        out["logits_sample_index"] = idx.astype(np.float64)
        out["logits_last"] = torch.cat([x[:, -1, :].float() for x in lg])[:DUMP_LAST_ROWS].cpu().numpy()
    if "sequences" in held:
        out["sequences"] = torch.cat(held["sequences"]).cpu().numpy().astype(np.float64)
    return out


def launch_roofline(m, step, n, kind):
    """Roofline block of a secondary line: `n` more steps of `step` with HIP events (on the launch stream) around every GEMM
    launch of model m's library, launched eagerly (the hook sits in the launch functions, not in replayed graphs).
    kind "mfma": the 256x256 MFMA GEMM against the dense peak of the operand type (bf16 / fp16 2.5 PF, e4m3 5 PF); for the
    reference-precision build the MFMA work is 3x the algorithmic flops (hi.hi + hi.lo + lo.hi) and both are reported.
    kind "hbm": the decode-step weight-streaming kernel against 8 TB/s (bytes = the N x K 16-bit weight, read once per launch)."""
    from groma_amd import engine, ops
    old_graph, old_pool = m.decode_graph, engine.GraphPool.enabled
    m.decode_graph, engine.GraphPool.enabled = False, False
    try:
        recs, vit_recs = profiled_steps(m, step, n, 1000)
    finally:
        m.decode_graph, engine.GraphPool.enabled = old_graph, old_pool
    if kind == "hbm":
        gv = [r for r in recs if r[3] & 8]
        ms = sum(r[4] for r in gv)
        nbytes = sum((1.0 if r[3] & 16 else 2.0) * r[1] * r[2] for r in gv)   # (tag 16: e4m3 weights, one byte per element)
        ach = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        return {"bound": "hbm", "kernel": _stream_kernel_name(bool(m.fp8)), "achieved": ach, "peak": 8000.0,
                "unit": "GB/s", "frac": ach / 8000.0, "traffic": None, "launches_per_step": len(gv) / n,
                "avg_launch_us": ms * 1e3 / max(len(gv), 1), "bytes_per_launch": nbytes / max(len(gv), 1)}
    fp8 = bool(m.fp8)
    dom = [r for r in recs if (r[3] & 16 if fp8 else (r[3] & 4 and not r[3] & 16))]
    ms = sum(r[4] for r in dom)
    fl = sum(2.0 * r[0] * r[1] * r[2] for r in dom)
    mult = 3.0 if m.precision == "ref" else 1.0
    peak = 5000.0 if fp8 else 2500.0
    ach = mult * fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    out = {"bound": "mfma", "kernel": ("gemm_fp8_256_kernel" if fp8 else "gemm_bf16_256_kernel") + "(GemmArgs)", "achieved": ach, "peak": peak,
           "unit": "TFLOP/s", "frac": ach / peak, "traffic": None, "launches_per_step": len(dom) / n,
           "avg_launch_us": ms * 1e3 / max(len(dom), 1), "flops_per_launch": mult * fl / max(len(dom), 1)}
    if mult != 1.0:
        out["note"] = ("operand pairs: every contraction issues hi.hi + hi.lo + lo.hi, so `achieved` counts 3x the algorithmic 2MNK "
                       "(the MFMA work actually issued); algorithmic rate = achieved / 3")
        out["algorithmic_tflops"] = ach / 3.0
    if vit_recs is not None:
        out["vit_pair_gemms"] = pair_block(vit_recs, n)
    return out


def _stream_kernel_name(fp8):
    """the decode step's weight-streaming kernel as it appears in a trace (csrc/gemv_fused.hip / csrc/gemv_fp8.hip)"""
    return ("gemv_fp8_kernel<MB>(GemvFArgs) -- e4m3 weight stream on the matrix unit" if fp8 else
            "gemv_fused_kernel<MB, XG>(GemvFArgs) -- 16-bit weight stream") + ", one launch per weight matrix"


def profiled_steps(m, step, n, base):
    """n eager steps with the HIP-event hook on in the library of every stage of model m -> (records of the library behind the
    ViT, records of the ViT's own library or None when it is the same one)"""
    from groma_amd import ops
    libs = [m.precision] + ([m.vit_precision] if m.vit_precision != m.precision else [])
    for p in libs:
        with ops.precision(p):
            ops.prof_enable(True)
    for i in range(n):
        step(base + i)
    torch.cuda.synchronize()
    out = []
    for p in libs:
        with ops.precision(p):
            ops.prof_enable(False)
            out.append(ops.prof_read_launches())
    return out[0], (out[1] if len(out) > 1 else None)


def pair_block(vit_recs, n):
    """the ViT's GEMMs of a precision="hybrid" model (libgroma_hip_ref.so: gemm_pair_256_kernel / gemm_pair_kernel, 3 MFMA passes on
    (hi, lo) operand pairs): issued MFMA work against the 2.5 PF peak, and the algorithmic rate (a third of it)"""
    ms = sum(r[4] for r in vit_recs)
    fl = sum(2.0 * r[0] * r[1] * r[2] for r in vit_recs)
    ach = 3.0 * fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    return {"kernels": "gemm_pair_256_kernel / gemm_pair_kernel (libgroma_hip_ref.so): hi.hi + hi.lo + lo.hi per contraction",
            "launches_per_step": len(vit_recs) / max(n, 1), "ms_per_step": ms / max(n, 1), "issued_tflops": ach, "frac_issued": ach / 2500.0,
            "algorithmic_tflops": ach / 3.0}


def extras_block(model, cfg, args, dev, P):
    """Secondary lines measured in the SAME run, after (outside) the headline's timed region, N = 1 only: the small-batch
    forward (SURVEY 8d configs[2] at 1 and 4 images per call), configs[3]'s per-GPU share (greedy generate, 4 images, 32 new
    tokens), configs[4] (e4m3 operands) and the fp16 operand build.  Each is its own ShardedJob.timed() with its own warm-up."""
    from groma_amd import constants, dist as gdist
    from groma_amd.groma import GromaModel
    ex = {}

    def line(m, batch, gen, plan="throughput", steps=10, warmup=3, roof=None):
        head = (P + args.new_tokens) if gen else 100
        job = gdist.ShardedJob(dev, (head + ROW_BOXES + 1,), torch.float32, rows_per_rank=batch)
        el, step = measure(m, cfg, args, dev, 0, job, P, gen, batch, plan=plan, steps=steps, warmup=warmup)
        out = {"value": batch * steps / el, "unit": "images/s", "ms_per_step": el / steps * 1e3, "images_per_call": batch,
               "gemm_plan": plan, "steps": steps, "warmup": warmup}
        if roof:
            old = m.gemm_plan
            m.gemm_plan = plan
            try:
                out["roofline"] = launch_roofline(m, step, 2, roof)
            finally:
                m.gemm_plan = old
            n_reg = [b.shape[0] for b in m._last_aux["sel_idx"]]
            tf = flops_per_image(cfg, sum(n_reg) / len(n_reg), P)["total"] * batch * steps / el / 1e12
            if not gen:
                out["e2e_algorithmic_tflops_per_gpu"] = tf
        return out

    ex["forward_1_image_per_call"] = line(model, 1, False)
    ex["forward_1_image_per_call_latency_plan"] = line(model, 1, False, plan="latency")
    ex["forward_4_images_per_call"] = line(model, 4, False, roof="mfma")
    ex["forward_4_images_per_call_latency_plan"] = line(model, 4, False, plan="latency")
    eos = model.generation_config.eos_token_id
    model.generation_config.eos_token_id = None
    try:
        g = line(model, 4, True, steps=3, warmup=3, roof="hbm")
    finally:
        model.generation_config.eos_token_id = eos
    def decode_step(m, g, pre_ms):
        """per decode step: (generate - prefill) / new tokens against the weight bytes every token streams once (13.2 GB 16-bit, 6.6 GB e4m3)"""
        g["new_tokens"] = args.new_tokens
        try:
            tok_ms = (g["ms_per_step"] - pre_ms) / max(args.new_tokens - 1, 1)
            head = m.llm.w["head8"][0] if (m.fp8 and "head8" in m.llm.w) else m.llm.w["head"]
            wbytes = sum(t.numel() * t.element_size() for L in m.llm.w["layers"] for t in (L["wqkv"][0], L["wo"][0], L["wgu"][0], L["wd"][0]))
            wbytes += head.numel() * head.element_size()
            g["decode_step"] = {"ms_per_token": tok_ms, "weight_bytes_per_token": wbytes, "hbm_GBps_end_to_end": wbytes / (tok_ms * 1e-3) / 1e9,
                                "frac_of_8TBps": wbytes / (tok_ms * 1e-3) / 8e12,
                                "note": "(generate ms - 4-image prefill ms) / (new_tokens - 1): everything a token costs, not only the weight-stream launches"}
        except Exception as e:
            g["decode_step"] = {"error": str(e)}
        g["workload"] = "configs[3] per-GPU share: prefill + greedy decode (hipGraph replay), no EOS"
        return g
    ex["generate_4_images_per_call"] = decode_step(model, g, ex["forward_4_images_per_call"]["ms_per_step"])
    # configs[3]'s WHOLE batch on one GPU (round 6): 32 rows decode on the matrix-unit weight stream (csrc/gemm_skinny.hip) -- the same
    # weight bytes per token as 4 rows, eight times the tokens
    eos = model.generation_config.eos_token_id
    model.generation_config.eos_token_id = None
    try:
        pre32 = line(model, 32, False, steps=3, warmup=3)
        g32 = line(model, 32, True, steps=2, warmup=3)
        g32["new_tokens"], g32["prefill_ms_32_images"] = args.new_tokens, pre32["ms_per_step"]
        g32["decode_step"] = {"ms_per_token": (g32["ms_per_step"] - pre32["ms_per_step"]) / max(args.new_tokens - 1, 1), "rows": 32,
                              "note": "(generate ms - 32-image prefill ms) / (new_tokens - 1): one tick of 32 rows"}
        g32["workload"] = "configs[3]'s global batch (32 images) in ONE generate() call on one GPU: prefill + greedy decode, 32 rows per tick"
        ex["generate_32_images_per_call"] = g32
    except Exception as e:
        ex["generate_32_images_per_call"] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    finally:
        model.generation_config.eos_token_id = eos
    def other(name, dtype_note, steps=5, gen_name=None, **kw):
        """a line measured on another model instance (built, measured, freed); gen_name: also its greedy generate at 4 images per call.
        A failure costs this line only (the error is reported in its place), never the lines already measured."""
        try:
            _other(name, dtype_note, steps, gen_name, **kw)
        except Exception as e:
            ex[name] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()

    def _other(name, dtype_note, steps, gen_name, **kw):
        m = GromaModel.from_synthetic(cfg, seed=0, device=dev, **kw)
        m.init_special_token_id(constants.SyntheticTokenizer())
        r = line(m, args.batch, False, steps=steps, warmup=3, roof="mfma")
        r["dtype"], r["precision"] = dtype_note, m.mode
        ex[name] = r
        if gen_name:
            m.generation_config.eos_token_id = None
            pre = line(m, 4, False, steps=5, warmup=3)
            gg = decode_step(m, line(m, 4, True, steps=3, warmup=3, roof="hbm"), pre["ms_per_step"])
            gg["dtype"], gg["precision"], gg["prefill_ms_4_images"] = dtype_note, m.mode, pre["ms_per_step"]
            ex[gen_name] = gg
        del m
        torch.cuda.empty_cache()

    # BASELINE configs[2]'s nominal dtype, both ways (always reported: ADVICE r05): round 5's headline (bf16 behind a pair-operand ViT:
    # index-valued results exact, logits at the bf16 format's distance) and rounds 1-4's (bf16 in every stage incl. the ViT)
    if model.mode != "hybrid":
        other("forward_hybrid_bf16", "precision='hybrid': the ViT on operand pairs, everything behind it on bf16 operands (round 5's headline: the "
              "index-valued results equal the fp32 reference's, the logits sit at 2.6e-2 at full depth)", precision="hybrid")
    other("forward_bf16_vit", "bf16 operands in every stage incl. the ViT (precision='bf16', rounds 1-4's headline): faster, but the proposer's ranking "
          "is no longer the fp32 reference's end to end (tests/test_e2e_unchained_gpu.py: 51-59 % of the top-300 slots)", precision="bf16")
    other("forward_fp8", "fp8: OCP e4m3 operands (MX-rate MFMA) for the LLaMA linears, lm_head and the region encoder's 3x3 / per-ROI convs, f32 "
          "accumulate; the ViT on operand pairs (precision='hybrid', fp8=True), so the e4m3 build holds the index contract too; its decode step streams "
          "the e4m3 bytes on the matrix unit (csrc/gemv_fp8.hip)", gen_name="generate_fp8_4_images_per_call", precision="hybrid", fp8=True)
    other("forward_fp8_e4m3_vit", "fp8 in every stage incl. the ViT linears (round 4's forward_fp8)", fp8=True)
    if model.mode != "hybrid-fp16":
        other("forward_fp16", "fp16 (IEEE half operands through libgroma_hip_f16.so, f32 accumulate: the reference's inference autocast dtype) behind a "
              "pair-operand ViT (precision='hybrid-fp16')", precision="hybrid-fp16")
    other("forward_ref", "ref: (hi, lo) pairs of halves through libgroma_hip_ref.so in EVERY stage, three MFMA passes per contraction, f32 accumulate -- "
          "the mode that also holds north_star's 1e-3 on the full-depth logits against the fp32 oracle (tests/test_fulldepth_parity_gpu.py)",
          steps=3, precision="ref")
    return ex


def parity_block(precision, fp8, images, ids, seed, n_images=4):
    """The benchmarked MODE checked against the oracle on the bench's OWN inputs: the first `n_images` images /
    prompts of the timed batch and the CPU-RNG seed of its first timed step, through a model of Groma-7B WIDTH at reduced depth
    (config.groma_7b_width: every GEMM / conv / attention shape of the benchmark, 3 ViT layers, 6+6 DDETR, 1 fusion round, 1 LLaMA
    layer -- the depth at which the fp32 oracle finishes in seconds; the full-depth figures are tests/test_fulldepth_parity_gpu.py's)
    built with the SAME per-stage operand types, against the fp32 oracle running its own fp32 ViT -- unchained, nothing of the device
    enters the oracle (R: groma/model/groma.py:222-280,317-402 in one fp32 pass).  Reported per image: whether the top-300 proposal
    ids / NMS keep ids / shuffled selection / spliced token ids are EQUAL, the oracle's smallest adjacent logit gap next to the
    device's class-logit error (a ranking only RESOLVES when gap > 2 err: two fp32 evaluations may order a closer pair either
    way), whether the device ranking is a valid ranking of the oracle's logits within 2 err, and the logits' relative L2 distance.
    These inputs are not selected for large gaps (tests/test_e2e_unchained_gpu.py's committed seeds are)."""
    import time
    from groma_amd import config as gconfig, constants, synth
    from groma_amd.groma import GromaModel
    from oracle import groma_oracle as O
    t0 = time.time()
    torch.set_num_threads(max(1, min(64, os.cpu_count() or 8)))
    cfg = gconfig.groma_7b_width(box_score_thres=0.0)
    sd = synth.make_state_dict(cfg, 0)
    m = GromaModel.from_state_dict(cfg, sd, images.device, fp8=fp8, precision=precision)
    m.init_special_token_id(constants.SyntheticTokenizer())
    n = min(n_images, images.shape[0])
    im, tok_ids = images[:n].float(), ids[:n]
    torch.manual_seed(seed)
    out = m.forward(input_ids=tok_ids.clone(), images=im, return_dict=True)
    aux = m._last_aux
    dbg = {}
    m.proposer.forward(aux["hidden4"], debug=dbg)
    d_cls = dbg["enc_class"].float().cpu()
    tok = dict(pad_token_id=m.pad_token_id, img_token_id=m.img_token_id, reg_token_id=m.reg_token_id,
               refer_box_token_id=m.refer_box_token_id, refer_feat_token_id=m.refer_feat_token_id,
               ground_box_token_id=m.ground_box_token_id, box_idx_token_ids=m.box_idx_token_ids)
    torch.manual_seed(seed)
    with torch.no_grad():
        ref = O.groma_forward(sd, cfg.to_dict(), tok, tok_ids.cpu().clone(), im.cpu())   # hidden_states=None: its own fp32 ViT
    o_cls = ref["det"]["enc_class"]
    Q = aux["topk_idx"].shape[1]
    d_ids, o_ids = aux["topk_idx"].cpu().long(), ref["det"]["topk_idx"]
    per = []
    for i in range(n):
        srt = torch.sort(o_cls[i], descending=True)[0][: Q + 1]
        gap = (srt[:-1] - srt[1:]).min().item()
        err = (d_cls[i] - o_cls[i]).abs().max().item()
        v = o_cls[i][d_ids[i]]
        rest = torch.ones_like(o_cls[i], dtype=torch.bool)
        rest[d_ids[i]] = False
        valid = bool((v[1:] - v[:-1]).max().item() <= 2 * err and (not rest.any() or o_cls[i][rest].max().item() <= v.min().item() + 2 * err))
        perm = ref["perms"][i]
        per.append({"top300_ids_equal": torch.equal(d_ids[i], o_ids[i]), "top300_slots_equal": (d_ids[i] == o_ids[i]).float().mean().item(),
                    "nms_ids_equal": torch.equal(aux["nms_keep"][i], ref["nms_inds"][i]),
                    "selection_equal": perm is not None and torch.equal(aux["sel_idx"][i], ref["nms_inds"][i][perm]),
                    "oracle_min_gap": gap, "class_logit_err": err, "resolves": gap > 2 * err, "valid_ranking_within_2err": valid})
    same = aux["input_ids"].shape == ref["input_ids"].shape
    lg_d, lg_o = out.logits.float().cpu(), ref["logits"]
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    ids_row_eq = [bool(same and torch.equal(aux["input_ids"][i], ref["input_ids"][i])) for i in range(n)]
    for i, pi in enumerate(per):
        pi["spliced_ids_equal"] = ids_row_eq[i]
        pi["all_index_results_equal"] = bool(pi["top300_ids_equal"] and pi["nms_ids_equal"] and pi["selection_equal"] and ids_row_eq[i])
        pi["logits_rel_l2"] = rel(lg_d[i], lg_o[i]) if same else None
    eq = [i for i, pi in enumerate(per) if pi["all_index_results_equal"]]
    tol = PARITY_TOL.get(m.mode.split("+")[0] + ("+e4m3" if fp8 else ""), None)
    res = {"mode": m.mode, "inputs": f"images / prompts 0..{n - 1} of the timed batch (seed 1234 + rank), CPU-RNG seed {seed} (the first timed step's)",
           "model": "Groma-7B width at reduced depth (3 ViT / 6+6 DDETR / 1 fusion round / 1 LLaMA layer), random-init seed 0",
           "oracle": "fp32 CPU restatement running its own fp32 ViT (unchained)",
           "images": per,
           "n_images": n, "images_with_all_index_results_equal": len(eq),
           # an image whose oracle ranking hangs on a gap below the fp32 evaluation error of either implementation (resolves = false) may
           # order that pair differently; its selected regions then differ and its logits are not comparable position by position
           "near_tie_images": [i for i, pi in enumerate(per) if not pi["all_index_results_equal"] and not pi["resolves"]],
           "unexplained_images": [i for i, pi in enumerate(per) if not pi["all_index_results_equal"] and (pi["resolves"] or not pi["valid_ranking_within_2err"])],
           "spliced_ids_equal": bool(same and torch.equal(aux["input_ids"], ref["input_ids"])),
           "vit_states_rel_l2": max(rel(h.float().cpu(), r) for h, r in zip(aux["hidden4"], ref["hidden_states"][-4:])),
           "logits_rel_l2": (rel(lg_d[eq], lg_o[eq]) if (same and eq) else None),
           "logits_rel_l2_note": "over the images whose index-valued results equal the oracle's (the others are near-ties: see images[].resolves)",
           "logits_rel_l2_all_images": rel(lg_d, lg_o) if same else None,
           "argmax_agree": ((lg_d[eq].argmax(-1) == lg_o[eq].argmax(-1)).float().mean().item() if (same and eq) else None),
           "logits_tolerance": tol,
           "seconds": round(time.time() - t0, 1)}
    res["all_index_results_equal"] = len(eq) == n
    res["within_tolerance"] = bool(res["logits_rel_l2"] is not None and tol is not None and res["logits_rel_l2"] <= tol and not res["unexplained_images"])
    del m, out
    torch.cuda.empty_cache()
    return res


# stated tolerance of the logits (relative L2 against the unchained fp32 oracle) at the parity block's reduced depth, per mode: the
# 16-bit format behind the ViT (measured 7.8e-3 bf16 / 9.8e-4 fp16 / 5e-6 pairs / ~9e-2 e4m3; full depth: DESIGN.md 4)
PARITY_TOL = {"hybrid": 1.5e-2, "bf16": 1.5e-2, "hybrid-fp16": 2e-3, "fp16": 2e-3, "ref": 1e-4, "hybrid+e4m3": 1.5e-1, "bf16+e4m3": 1.5e-1}


# The headline's 16-bit operand type (round 6).  BASELINE configs[2] says "bf16"; the contract says dtype >= the reference's and the
# north star asks for logits within a stated tolerance of the reference's fp32 pass.  Measured at full depth, unchained
# (profiles/r06_precision_ablation.txt): hybrid (bf16) 2.6e-2, hybrid-fp16 3.3e-3 -- same MFMA rate, same bytes, 3 % slower (the half
# MFMA's clock / issue price) -- and no stage set under 2.4x the step reaches 1e-3.  IEEE half is also the dtype the
# reference's own inference entry points autocast to (R: groma/eval/run_groma.py:82, groma/serve/model_worker.py:256).
HEADLINE_DTYPE = "fp16"


def extras_summary(ex):
    """{line: [images/s, roofline fraction of its dominant kernel or None]} + the decode step: what the driver's stored head / tail
    of the JSON line must still show (the long extras block is cut out of the middle)"""
    out = {}
    for k, v in (ex or {}).items():
        if isinstance(v, dict) and "value" in v:
            rf = v.get("roofline") or {}
            out[k] = [round(v["value"], 2), round(rf["frac"], 3) if "frac" in rf else None]
            if "decode_step" in v and "ms_per_token" in v["decode_step"]:
                tag = "decode_fp8" if "fp8" in k else ("decode_32_rows" if "_32_" in k else "decode")
                fr = v["decode_step"].get("frac_of_8TBps")
                out[tag + "_ms_per_token"] = [round(v["decode_step"]["ms_per_token"], 3), round(fr, 3) if fr is not None else None]
    return out


def pin_host_threads(local_rank, world):
    """One rank per GPU shares the host with world - 1 others: give each rank its own contiguous slice of the cores it may run
    on (affinity) and size torch's intra-op pool to it, so the ranks' host glue around the NMS sync (randperm, splice, pinned
    copies) does not contend for the same cores.  Returns the thread count in effect.  N = 1: untouched."""
    if world <= 1:
        return torch.get_num_threads()
    try:
        cores = sorted(os.sched_getaffinity(0))
        per = max(1, len(cores) // world)
        mine = cores[local_rank * per:(local_rank + 1) * per] or cores
        os.sched_setaffinity(0, mine)
        torch.set_num_threads(max(1, min(len(mine), 16)))
    except (AttributeError, OSError):
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
    return torch.get_num_threads()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3,
                    help="untimed steps (3 or more: a prefill graph is captured the third time its shape is seen)")
    ap.add_argument("--batch", type=int, default=14, help="images per GPU per step (14*582 = 8148 rows ~ 32 GEMM row-tiles of 256)")
    ap.add_argument("--config", default="7b", choices=["7b", "tiny"])
    ap.add_argument("--dtype", default=HEADLINE_DTYPE, choices=["bf16", "fp16", "fp8"],
                    help="16-bit operand type of everything behind the ViT.  fp16 is the headline since round 6 (same MFMA rate as bf16, 3 "
                         "more mantissa bits: the build whose logits are closest to the reference's fp32 pass at >= 0.40 of peak -- "
                         "profiles/r06_precision_ablation.txt; bf16, BASELINE configs[2]'s nominal dtype, is reported beside it in "
                         "`extras` and `summary_tail`); fp16 = the "
                         "IEEE-half build of the same kernels (libgroma_hip_f16.so: the reference's own inference autocast dtype, "
                         "same MFMA rate); fp8 = OCP e4m3 operands + f32 accumulate (BASELINE configs[4] extension)")
    ap.add_argument("--vit-operands", default="pair", choices=["pair", "same"],
                    help="pair (default, GromaModel precision='hybrid'): the DINOv2 encoder runs on (hi, lo) half pairs with three MFMA "
                         "passes per contraction (libgroma_hip_ref.so), which makes the proposal / NMS / token ids of the run equal the "
                         "fp32 reference's; same: the ViT uses --dtype operands like every other stage (the headline of rounds 1-4)")
    ap.add_argument("--mode", default="forward", choices=["forward", "generate"],
                    help="forward = the headline prefill metric (BASELINE configs[2]); generate = configs[3]: greedy decoding "
                         "of --new-tokens tokens per image at --batch images per GPU (use --batch 4), HBM-bound decode steps")
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the RCCL process group and run the per-step all-gather even with one rank (smoke test of "
                         "the N>1 path on a 1-GPU box)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="STRONG scaling: a fixed number of images per step, sharded over the ranks (groma_amd.dist.shard_range) and "
                         "processed in micro-batches of --batch.  BASELINE configs[3] = --mode generate --global-batch 32 --batch 4 "
                         "(4 images per GPU at 8 ranks).  0 (default) = weak scaling, --batch images on every rank")
    ap.add_argument("--gemm-plan", default="throughput", choices=["throughput", "latency"],
                    help="split-K plan class of the headline measurement (ops.plan_splits): a function of the layer shape only")
    ap.add_argument("--no-prefill-graphs", action="store_true",
                    help="launch the ViT / LLaMA prefill layers eagerly instead of replaying their captured hipGraphs (A/B)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure everything else the benchmark reports: the per-kernel roofline (the same steps "
                         "again, eagerly, with HIP events), the live PMC traffic passes, `extras` (other batch sizes, plans, precisions, "
                         "generate), the `parity` block and the CPU baseline.  Off: set up, warm up, time the steps, dump, print")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-parity", action="store_true",
                    help="with --full: skip the `parity` block (the benchmarked mode against the unchained fp32 oracle on the bench's own "
                         "inputs at reduced depth: N = 1, rank 0, after the timed region)")
    ap.add_argument("--no-traffic", action="store_true",
                    help="with --full: skip the live rocprofv3 PMC passes for roofline.traffic (the committed profiles/ summary is reported instead)")
    ap.add_argument("--generate-traffic", action="store_true",
                    help="with --full --mode generate: also run the rocprofv3 PMC passes for the stream kernel's traffic (OFF by default: the profiler crashes or hangs "
                         "on the generate run on this image -- round 6 lost two 5-minute timeouts to it; the round-5 figure stands: 103.7 MB per launch against 102.5 algorithmic)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the `extras` block (1 and 4 images per call, greedy generate, e4m3 operands: measured after the "
                         "headline's timed region, N = 1 only)")
    ap.add_argument("--cpu-baseline-reps", type=int, default=3,
                    help="with --full: timed full-depth oracle forwards after the reduced-depth warm-up; the median is reported (BASELINE.md 3)")
    ap.add_argument("--gemm-breakdown", default=None,
                    help="with --full: write a per-shape GEMM table (from the HIP-event hook of the roofline leg) here")
    ap.add_argument("--host-glue", action="store_true",
                    help="with --dry-exchange: every rank also runs the forward's real host-side glue (CPU-RNG shuffles, placeholder "
                         "splice, scatter-row lists) per step and the JSON reports its microseconds per step under N-way host contention")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step handed its caller as DIR/<name>.npy (float32 / float64, rank 0, <= 64 MB; "
                         "a fixed sample of the full logits: see dump_arrays) -- the inputs are seeded, so two builds compare output for output")
    ap.add_argument("--dry-exchange", action="store_true",
                    help="launcher / process-group / exchange / timing path only, with synthetic rows on CPU (gloo); no model")
    args = ap.parse_args()

    if args.gemm_breakdown and not args.full:
        ap.error("--gemm-breakdown needs --full (the table comes from the roofline leg)")
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one process per GPU (or let `python bench.py --gpus N` do it)")
    if args.dry_exchange:
        pin_host_threads(local_rank, world)
        raise SystemExit(run_dry_exchange(args, rank, world))
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but {torch.cuda.device_count()} GPU(s) visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    host_threads = pin_host_threads(local_rank, world)

    from groma_amd import config as gconfig, constants, dist as gdist, engine, ops, synth
    from groma_amd.groma import GromaModel
    engine.GraphPool.enabled = not args.no_prefill_graphs
    if use_dist:
        gdist.init("nccl", dev, single_process=(world == 1))  # RCCL over xGMI; rendezvous on 127.0.0.1 unless the launcher says otherwise
    rccl_ranks = gdist.count_ranks(dev)  # all-reduce of ones: proves how many ranks took part (1 without a process group)
    if rccl_ranks != world:
        raise SystemExit(f"process group has {rccl_ranks} ranks, expected {world}")

    cfg = gconfig.groma_7b(box_score_thres=0.0) if args.config == "7b" else gconfig.groma_tiny(box_score_thres=0.0)
    fp8 = args.dtype == "fp8"
    precision = "fp16" if args.dtype == "fp16" else "bf16"
    ops._lib.PRECISION[0] = precision  # process default = the library of everything behind the ViT (the HIP-event hook is per library)
    pair_vit = args.vit_operands == "pair"
    # the headline build since round 5 is precision="hybrid": the ViT -- the one 16-bit stage in front of the fp32 proposer -- on (hi, lo)
    # operand pairs, so that the top-300 / NMS / spliced ids of the benchmarked build equal the fp32 reference's end to end
    # (tests/test_e2e_unchained_gpu.py); everything behind it on --dtype operands.  --vit-operands same = rounds 1-4's headline.
    model = GromaModel.from_synthetic(cfg, seed=0, device=dev, fp8=fp8, precision={"bf16": "hybrid", "fp16": "hybrid-fp16"}[precision] if pair_vit else precision)
    model.init_special_token_id(constants.SyntheticTokenizer())
    P = 128
    gen = args.mode == "generate"
    strong = args.global_batch > 0
    # the per-rank driver (shard bookkeeping, ONE all-gather of the per-image rows per step, barrier + max-over-ranks
    # timing) is groma_amd.dist.ShardedJob -- the same code tests/test_dist_gloo.py runs with 2 gloo ranks.  A row carries
    # everything SURVEY 8e lists: region logits (or generated ids), pred_boxes [100, 4], N_i
    head_w = (P + args.new_tokens) if gen else 100
    job = gdist.ShardedJob(dev, (head_w + ROW_BOXES + 1,), torch.float32,
                           **(dict(global_batch=args.global_batch) if strong else dict(rows_per_rank=args.batch)))
    if gen:
        model.generation_config.eos_token_id = None  # random-init weights: fixed-length decode, never an early stop

    dumped = {} if args.dump_outputs and rank == 0 else None
    elapsed, step = measure(model, cfg, args, dev, rank, job, P, gen, args.batch, plan=args.gemm_plan, strong=strong, keep=dumped)
    if dumped is not None:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dumped.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    gathered = job.last_rows   # what the exchange delivered at the last timed step
    exchanged_regions = int(gathered[:, -1].sum().item())
    n_reg = [b.shape[0] for b in model._last_aux["sel_idx"]] if job.rows else [100]
    fl = flops_per_image(cfg, sum(n_reg) / len(n_reg), P)
    ips = job.global_batch * args.steps / elapsed
    peak = 5000.0 if fp8 else 2500.0  # dense MFMA peak of the operand type (MI355X_MICROARCH.md)
    out = {
        "metric": "images/sec end-to-end forward (448px, 300 proposals, 128 tok)",
        "value": ips, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "dtype_note": ("IEEE half operands (f32 accumulate, fp32 residual streams) behind a pair-operand ViT: same MFMA rate and bytes as BASELINE's bf16, 3 more "
                       "mantissa bits -- full-depth logits 3.3e-3 from the reference's fp32 pass instead of bf16's 2.6e-2 (profiles/r06_precision_ablation.txt); "
                       "the bf16 builds are in extras / summary_tail (--full)") if args.dtype == "fp16" else None,
        "rccl_ranks": rccl_ranks,  # all-reduce of ones over the process group: the ranks that actually took part
        # the slowest / fastest rank's own time per step (max is what `value` is computed from): load imbalance across ranks
        "ms_per_step_rank_max": job.last_elapsed_max / args.steps * 1e3, "ms_per_step_rank_min": job.last_elapsed_min / args.steps * 1e3,
        "graph_captures_in_timed_region": job.captures_in_timed_region, "graph_setup_steps": getattr(job, "setup_steps", 0),
        "host_threads_per_rank": host_threads,
        "full": args.full,
        "exchange": {"collective": "one all_gather_into_tensor per step" if use_dist else "none (single process)",
                     "row_f32": {"head": head_w, "pred_boxes": ROW_BOXES, "n_regions": 1},
                     "rows_gathered": int(gathered.shape[0]), "regions_gathered": exchanged_regions},
        "config": {"workload": "configs[2]: full Groma-7B forward (DINOv2-L + DDETR 300 proposals -> NMS 100 regions + "
                               "region encoder + Vicuna-7B prefill, logits for all positions), random-init weights"
                               if args.config == "7b" else "tiny parity architecture (NOT the headline workload)",
                   "images_per_gpu": job.rows, "images_per_forward_call": min(args.batch, job.rows),
                   "global_batch": job.global_batch, "prompt_tokens": P,
                   "llm_seq_len": fl["L"], "regions_per_image": sum(n_reg) / len(n_reg),
                   "precision": model.mode,
                   "vit_operands": ("(hi, lo) pairs of halves, 3 MFMA passes per contraction (libgroma_hip_ref.so): the index-valued results of "
                                    "this build equal the fp32 reference's, unchained" if model.vit_precision == "ref" else "same as dtype"),
                   "gemm_plan": args.gemm_plan, "prefill_graphs": not args.no_prefill_graphs,
                   "parallelism": f"dp{world} (image batch sharded, full replica per GPU)"},
        # the flop model over the headline's own time; the per-kernel figures need a leg of their own (--full)
        "roofline": {"bound": "mfma", "peak": peak, "unit": "TFLOP/s",
                     "e2e_algorithmic_tflops_per_gpu": fl["total"] * job.rows * args.steps / elapsed / 1e12,
                     "e2e_frac_of_peak": fl["total"] * job.rows * args.steps / elapsed / 1e12 / peak},
    }
    if dumped is not None:
        out["dump_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "step": args.warmup + args.steps - 1,
                               "arrays": {k: [str(a.dtype)] + list(a.shape) for k, a in dumped.items()},
                               "bytes": sum(a.nbytes for a in dumped.values())}
    if gen:
        out["metric"] = "images/sec greedy generate (448px, 300 proposals, 128-token prompt, %d new tokens)" % args.new_tokens
        out["config"]["workload"] = ("configs[3]: generate() = full Groma-7B prefill + %d greedy decode steps (hipGraph replay), "
                                     "random-init weights, no EOS" % args.new_tokens)
        out["config"]["new_tokens"] = args.new_tokens
        del out["roofline"]   # a forward's flop model says nothing about the decode steps: their HBM roofline is --full's
    if args.full:
        out = full_legs(out, model, cfg, args, dev, rank, world, job, step, elapsed, fl, P, fp8, gen)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if use_dist:
        import torch.distributed as dist
        dist.destroy_process_group()


def full_legs(out, model, cfg, args, dev, rank, world, job, step, elapsed, fl, P, fp8, gen):
    """--full: everything the JSON line carries beyond the headline, each leg after (outside) the timed region -- the roofline leg
    (the headline's steps again, eagerly, with HIP events around every GEMM launch), the PMC traffic passes, and on rank 0 of a
    one-GPU run the `extras`, `parity` and `cpu_baseline` blocks.  Every rank runs the roofline leg (its steps exchange)."""
    from groma_amd import engine
    from groma_amd import synth as _synth
    model.gemm_plan = args.gemm_plan

    # ---- roofline leg: the same steps again with HIP events around every GEMM launch (on the launch stream) ----
    # HIP events cannot bracket launches inside a replayed graph (the hook sits in the launch functions): time the same
    # kernels eagerly
    model.decode_graph = False
    engine.GraphPool.enabled = False
    recs, vit_recs = profiled_steps(model, step, args.steps, args.warmup)
    engine.GraphPool.enabled = not args.no_prefill_graphs
    model.decode_graph = True
    if args.gemm_breakdown and rank == 0:
        agg = {}
        for M_, N_, K_, tag, ms in recs:
            a = agg.setdefault((M_, N_, K_, tag), [0, 0.0])
            a[0] += 1
            a[1] += ms
        with open(args.gemm_breakdown, "w") as f:
            f.write("M N K tag(1=conv,2=splitK,4=ping-pong kernel,8=decode-step weight stream,16=e4m3,32=fused stream kernel) calls_per_step avg_us TFLOPs share_of_gemm_time\n")
            tot = sum(v[1] for v in agg.values())
            for (M_, N_, K_, tag), (c, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                f.write(f"{M_} {N_} {K_} {tag} {c / args.steps:.1f} {ms / c * 1e3:.1f} "
                        f"{2.0 * M_ * N_ * K_ * c / (ms * 1e-3) / 1e12:.0f} {ms / tot:.3f}\n")
    all_ms = sum(r[4] for r in recs)
    all_flops = sum(2.0 * r[0] * r[1] * r[2] for r in recs)
    dom = [r for r in recs if (r[3] & 16 if fp8 else (r[3] & 4 and not r[3] & 16))]  # the dominant kernel
    gemm_ms = sum(r[4] for r in dom)
    gemm_launches = len(dom)
    gemm_flops = sum(2.0 * r[0] * r[1] * r[2] for r in dom)
    # HBM-side traffic of the dominant kernel: measured live by two rocprofv3 --pmc child runs of this command (rank 0, one
    # GPU, forward mode); if the profiler cannot run here, the newest committed summary of the same passes is reported and
    # `traffic_source` says so
    traffic, traffic_source = None, None
    if rank == 0 and world == 1 and not args.no_traffic and args.config == "7b" and not fp8 and not gen:
        traffic = measure_traffic(args.batch, extra=["--vit-operands", args.vit_operands, "--dtype", args.dtype, "--no-parity"])
        if traffic is not None:
            traffic_source = "measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (separate child runs, gfx950 x2 fetch correction)"
    if traffic is None and args.config == "7b" and not fp8 and not gen:
        try:
            import glob
            cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic_b{args.batch}.json")))
            if cands:
                with open(cands[-1]) as f:
                    traffic = json.load(f)["kernels"]["gemm_bf16_256_kernel(GemmArgs)"]["traffic_bytes_per_launch"]
                traffic_source = "committed summary of the same rocprofv3 passes: profiles/" + os.path.basename(cands[-1])
        except Exception:
            traffic = None
    ips = out["value"]
    peak = 5000.0 if fp8 else 2500.0
    kname = "gemm_fp8_256_kernel(GemmArgs) -- 256x256 ping-pong e4m3 MFMA GEMM" if fp8 else \
        "gemm_bf16_256_kernel(GemmArgs) -- 256x256 ping-pong MFMA GEMM incl. implicit-GEMM 3x3 convs"
    achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    out["roofline"] = {"bound": "mfma", "kernel": kname,
                       "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak, "traffic": traffic,
                       "traffic_note": ("bytes/launch of gemm_bf16_256_kernel at the L2<->fabric boundary (Infinity-Cache hits "
                                        "included; DESIGN.md 3a); " + traffic_source) if traffic else None,
                       "launches_per_step": gemm_launches / max(args.steps, 1),
                       "avg_launch_us": gemm_ms * 1e3 / max(gemm_launches, 1),
                       "flops_per_launch": gemm_flops / max(gemm_launches, 1),
                       "kernel_time_share_of_step": (gemm_ms / args.steps) / (elapsed / args.steps * 1e3),
                       "all_gemm_kernels": {"achieved": all_flops / (all_ms * 1e-3) / 1e12 if all_ms > 0 else 0.0,
                                            "launches_per_step": len(recs) / max(args.steps, 1),
                                            "time_share_of_step": (all_ms / args.steps) / (elapsed / args.steps * 1e3)},
                       "e2e_algorithmic_tflops_per_gpu": fl["total"] * job.rows * args.steps / elapsed / 1e12,
                       "e2e_frac_of_peak": fl["total"] * job.rows * args.steps / elapsed / 1e12 / peak}
    if vit_recs is not None:
        out["roofline"]["vit_pair_gemms"] = pair_block(vit_recs, args.steps)
    if gen:  # configs[3]: the decode steps stream the bf16 weights once per token -> HBM roofline of the GEMV kernel
        gv = [r for r in recs if r[3] & 8]
        gv_ms = sum(r[4] for r in gv)
        gv_bytes = sum((1.0 if r[3] & 16 else 2.0) * r[1] * r[2] for r in gv)  # algorithmic bytes per launch: the N x K weight (16-bit, or e4m3 bytes: tag 16), read once
        ach = gv_bytes / (gv_ms * 1e-3) / 1e9 if gv_ms > 0 else 0.0
        gv_traffic = None
        if rank == 0 and world == 1 and not args.no_traffic and args.generate_traffic and args.config == "7b" and not fp8:
            # FETCH_SIZE / WRITE_SIZE of the fused weight-streaming kernel, per launch, from two rocprofv3 --pmc child runs of this
            # command (the decode steps are graph replays there; the counters see the same kernels)
            gv_traffic = measure_traffic(args.batch, "gemv_fused_kernel", ["--mode", "generate", "--new-tokens", str(args.new_tokens),
                                                                             "--vit-operands", args.vit_operands, "--dtype", args.dtype])
        out["roofline"] = {"bound": "hbm", "kernel": _stream_kernel_name(fp8),
                           "achieved": ach, "peak": 8000.0, "unit": "GB/s", "frac": ach / 8000.0, "traffic": gv_traffic,
                           "traffic_note": "bytes/launch at the L2<->fabric boundary (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, gfx950 correction), averaged over the fused-stream launches; algorithmic = bytes_per_launch" if gv_traffic else None,
                           "launches_per_step": len(gv) / max(args.steps, 1),
                           "avg_launch_us": gv_ms * 1e3 / max(len(gv), 1),
                           "bytes_per_launch": gv_bytes / max(len(gv), 1),
                           "kernel_time_share_of_step": (gv_ms / args.steps) / (elapsed / args.steps * 1e3)}
    if rank == 0:
        if world == 1 and not args.no_extras and not gen and args.dtype == HEADLINE_DTYPE:
            try:
                out["extras"] = extras_block(model, cfg, args, dev, P)
            except Exception as e:  # an extra never takes the headline down
                out["extras"] = {"error": f"{type(e).__name__}: {e}"}
            summ = extras_summary(out["extras"])
            # a compact copy at the FRONT (right behind the headline numbers) and again as the LAST key of the line
            out = dict(list(out.items())[:5] + [("extras_summary", summ)] + list(out.items())[5:])
        if world == 1 and not args.no_parity and not gen and args.config == "7b":
            try:   # the benchmarked MODE against the oracle on the bench's own inputs (reduced depth; see parity_block)
                p_im, p_ids = _synth.make_inputs(cfg, model, job.rows, seed=1234 + rank, prompt_len=P)   # exactly what measure() timed
                out["parity"] = parity_block(model.mode.replace("+e4m3", ""), fp8, p_im[:4].to(dev), p_ids[:4].to(dev), seed=1000 + args.warmup)
            except Exception as e:
                out["parity"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and not args.no_cpu_baseline and not gen:
            try:
                out["cpu_baseline"] = cpu_baseline(args.config, full_reps=args.cpu_baseline_reps)
            except Exception as e:  # never lose the GPU measurement to a host-side failure
                out["cpu_baseline"] = {"value": None, "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
                                       "sample": f"failed: {type(e).__name__}: {e}"}
        if "extras_summary" in out:
            exs = out.get("extras", {}) if isinstance(out.get("extras"), dict) else {}
            out["summary_tail"] = {"value": round(ips, 2), "precision": model.mode, "roofline_frac": round(achieved / peak, 4),
                                   "e2e_frac_of_peak": round(out["roofline"].get("e2e_frac_of_peak", 0.0), 4),
                                   # BASELINE configs[2]'s nominal dtype, unconditionally beside the headline (images/s)
                                   "bf16_operands_images_per_s": {"hybrid (pair ViT + bf16, round 5's headline)": round(exs.get("forward_hybrid_bf16", {}).get("value", 0.0), 2) or None,
                                                                  "bf16 in every stage (rounds 1-4's headline)": round(exs.get("forward_bf16_vit", {}).get("value", 0.0), 2) or None},
                                   "parity": {k: out.get("parity", {}).get(k) for k in ("n_images", "images_with_all_index_results_equal", "near_tie_images", "unexplained_images",
                                                                                        "logits_rel_l2", "logits_tolerance", "within_tolerance")},
                                   "extras [images/s, roofline frac]": out["extras_summary"]}
    return out


if __name__ == "__main__":
    main()
