"""Paged vs slot KV cache on Groma-7B (random init, full width and depth).

  python tests/diag/paged_kv_ab.py tick [--rows 8,32,64] [--ctx 600,4000] [--reps 3] [--slot-only]
      decode tick (one captured step of every row, LlamaEngine.forward at L = 1) over a slot cache and over a paged cache holding the
      same context per row, the two modes alternated in one process; each (mode, rows, ctx) cache is allocated, captured, timed
      (20 replays) and freed in turn, so a 64 x 4000 pair never needs both caches at once.  Median over --reps.
      --slot-only: the slot mode alone (for the same tick on another tree).
  python tests/diag/paged_kv_ab.py attn
      gr_decode_attention vs gr_decode_attention_paged at 7B shapes (32 heads x 128), 32 rows x 4000 keys: for a kernel trace.
  python tests/diag/paged_kv_ab.py serve [--pages 2048]
      ContinuousBatcher(max_rows=64, max_len=4096, kv_pages=N) on a mixed trace: REC requests (3 new tokens) and chat requests
      (512 new tokens); kv_stats() and img/s.
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def model7b():
    from groma_amd import config, constants
    from groma_amd.groma import GromaModel
    cfg = config.groma_7b(box_score_thres=0.0)
    m = GromaModel.from_synthetic(cfg, seed=0, device="cuda")
    m.init_special_token_id(constants.SyntheticTokenizer())
    m.generation_config.eos_token_id = None
    return cfg, m


def tick_ms(llm, rows, ctx, paged):
    """one captured decode step of `rows` rows at position ctx over a fresh cache; median of 20 timed replays (ms)"""
    from groma_amd import ops
    smax = -(-(ctx + 1) // 64) * 64
    dev = "cuda"
    if paged:
        per = smax // 64
        cache = llm.new_paged_cache(rows, smax, rows * per, dev)
        # row b owns pages b, b + rows, b + 2 rows, ... (+1 for the sink): interleaved, as a live pool would be after churn
        cache.table.copy_((torch.arange(per, device=dev)[None, :] * rows + torch.arange(rows, device=dev)[:, None] + 1).int())
    else:
        cache = llm.new_cache(rows, smax, dev)
    pos = torch.full((rows,), ctx, dtype=torch.int32, device=dev)
    h = torch.zeros((rows, llm.T), dtype=torch.float32, device=dev)
    with ops.precision("bf16"):
        for _ in range(3):
            llm.forward(h, rows, 1, cache, pos_dev=pos, pos_stride=1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            llm.forward(h, rows, 1, cache, pos_dev=pos, pos_stride=1)
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    del g, cache
    torch.cuda.empty_cache()
    return statistics.median(ts)


def run_tick():
    cfg, m = model7b()
    rows_list = [int(x) for x in arg("--rows", "8,32,64").split(",")]
    ctx_list = [int(x) for x in arg("--ctx", "600,4000").split(",")]
    reps = int(arg("--reps", 3))
    modes = (False,) if "--slot-only" in sys.argv else (False, True)
    print(f"decode tick, Groma-7B width, {len(m.llm.w['layers'])} layers, bf16; median of 20 replays per run, median of {reps} runs "
          f"(modes alternated)", flush=True)
    for rows in rows_list:
        for ctx in ctx_list:
            got = {md: [] for md in modes}
            for _ in range(reps):
                for md in modes:
                    got[md].append(tick_ms(m.llm, rows, ctx, md))
            line = f"rows={rows:3d} ctx={ctx:5d}  slot {statistics.median(got[False]):7.3f} ms  (runs {' '.join(f'{x:.3f}' for x in got[False])})"
            if True in got:
                p = statistics.median(got[True])
                line += (f"  paged {p:7.3f} ms  (runs {' '.join(f'{x:.3f}' for x in got[True])})"
                         f"  paged/slot {p / statistics.median(got[False]):.4f}")
            print(line, flush=True)


def run_attn():
    from groma_amd import ops
    B, H, hd, ctx = 32, 32, 128, 4000
    S = -(-(ctx + 1) // 64) * 64
    bf = torch.bfloat16
    k = torch.randn((B, H, S, hd), device="cuda").to(bf)
    vt = torch.randn((B, H, hd, S), device="cuda").to(bf)
    per = S // 64
    kp = torch.randn((B * per + 1, H, 64, hd), device="cuda").to(bf)
    vp = torch.randn((B * per + 1, H, hd, 64), device="cuda").to(bf)
    table = (torch.arange(per, device="cuda")[None, :] * B + torch.arange(B, device="cuda")[:, None] + 1).int()
    q = torch.randn((B, H, 1, hd), device="cuda").to(bf)
    out = torch.empty((B, H * hd), dtype=bf, device="cuda")
    pos = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    for _ in range(50):
        ops.decode_attention(q, k, vt, out, Smax=S, pos_dev=pos, pos_stride=1)
        ops.decode_attention_paged(q, kp, vp, out, table, Smax=S, pos_dev=pos, pos_stride=1)
    torch.cuda.synchronize()
    print(f"attn: {B} rows x {H} heads x {ctx + 1} keys, slot and paged x 50 each", flush=True)


def run_serve():
    from groma_amd import synth
    from groma_amd.serving import ContinuousBatcher
    cfg, m = model7b()
    pages = int(arg("--pages", 2048))
    b = ContinuousBatcher(m, max_rows=64, max_len=4096, kv_pages=pages)
    b.step()   # capture
    R = int(arg("--requests", 128))
    images, ids = synth.make_inputs(cfg, m, 16, seed=5)
    images = images.cuda()
    new = [3 if i % 2 == 0 else 512 for i in range(R)]   # REC and chat interleaved
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(R):
        b.submit(ids[i % 16], images[i % 16], max_new_tokens=new[i], seed=i)
    peak_rows = 0
    while b.queue or b.slots.active() or b._job is not None:
        b.step()
        peak_rows = max(peak_rows, len(b.slots.active()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    res = {rid: b.result(rid) for rid in list(b.live)}
    err = sum(r.error is not None for r in res.values())
    ntok = sum(len(r.tokens) for r in res.values())
    st = b.kv_stats()
    print(f"serve: ContinuousBatcher(max_rows=64, max_len=4096, kv_pages={pages}): {R} requests ({R // 2} x 3 + {R - R // 2} x 512 new "
          f"tokens) in {dt:.2f} s -> {R / dt:.1f} img/s, {ntok / dt:.0f} tok/s, {b.steps} ticks, peak {peak_rows} concurrent rows, "
          f"{err} errors", flush=True)
    print(f"kv_stats: pages_total={st['pages_total']} pages_free={st['pages_free']} high_water={st['high_water']} "
          f"pool={st['pool_bytes'] / 2**30:.2f} GiB staging={st['staging_bytes'] / 2**30:.2f} GiB; a slot arena of 64 x 4096 would be "
          f"{64 * 4096 * 32 * 2 * 4096 * 2 / 2**30:.0f} GiB + the same again for its staging cache", flush=True)


if __name__ == "__main__":
    {"tick": run_tick, "attn": run_attn, "serve": run_serve}[sys.argv[1]]()
