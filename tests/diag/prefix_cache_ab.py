"""Prefix cache on / off in the paged continuous batcher at Groma-7B width (random init, full width and depth).

  python tests/diag/prefix_cache_ab.py [--reps 2] [--pages 768]

Traffic: 8 images x 7 queries each (the REC shape: ~7 referring expressions per image), every query of an image with the image's seed,
a shared prompt head (system text, <image>, <region>, fixed turn) and its own 20..60-id tail.  Queued expression-major (the first query
of every image, then the second ...), as an eval loop over expressions submits them.  For max_new_tokens 3 (REC) and 32 (chat) and
max_rows 8 and 32: ContinuousBatcher(kv_pages=N) with prefix_cache off and on, alternated in one process (--reps rounds); requests/s,
mean admission wall time per request (the prefill calls, cold and suffix), and the suffix-prefill wall time per wave.  Then the
kernel times of gr_attention_paged and gr_attention_bf16 over the same keys (8 rows x 32 heads x 128, 64 queries at position 512).
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
    tk = constants.SyntheticTokenizer()
    m.init_special_token_id(tk)
    m.generation_config.eos_token_id = None
    return cfg, m


def traffic(cfg, m, n_img=8, n_q=7):
    from groma_amd import synth
    g = torch.Generator().manual_seed(1)
    V = cfg.llm_cfg.vocab_size
    reqs = []
    for i in range(n_img):
        images, _ = synth.make_inputs(cfg, m, bs=1, seed=500 + i)
        r = lambda n: torch.randint(3, V, (n,), generator=g)
        head = torch.cat([torch.tensor([1]), r(40), torch.tensor([m.img_token_id]), r(4), torch.tensor([m.reg_token_id]), r(30)])
        for j in range(n_q):
            reqs.append((j, i, torch.cat([head, r(20 + (37 * (i + j)) % 41)]), images[0], 900 + i))
    reqs.sort(key=lambda t: (t[0], t[1]))        # expression-major
    return [(ids, img, seed) for _, _, ids, img, seed in reqs]


def serve(m, reqs, rows, new, pages, cache):
    from groma_amd.serving import ContinuousBatcher
    b = ContinuousBatcher(m, max_rows=rows, max_len=1024, kv_pages=pages, prefix_cache=cache)
    b.warm_admission(reqs[0][0], reqs[0][1], rows=b.admit_rows)
    adm, sfx = [], []
    pre, pre_hits = b._prefill, b._prefill_hits

    def timed(reqs_):
        t0 = time.perf_counter()
        out = pre(reqs_)          # (first tokens are read back on the host: the wave has finished when this returns)
        adm.append((len(reqs_), time.perf_counter() - t0))
        return out

    def timed_hits(reqs_):
        t0 = time.perf_counter()
        out = pre_hits(reqs_)
        sfx.append((len(reqs_), time.perf_counter() - t0))
        return out
    b._prefill, b._prefill_hits = timed, timed_hits
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [b.submit(ids, img, max_new_tokens=new, seed=s) for ids, img, s in reqs]
    res = b.run_until_done()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    toks = [res[r].tokens for r in rids]
    assert all(res[r].error is None for r in rids)
    st = b.kv_stats()
    n = len(reqs)
    out = dict(rps=n / wall, adm_ms=1e3 * sum(t for _, t in adm) / n, waves=len(adm), hits=st["prefix_hits"],
               sfx_ms=1e3 * statistics.mean(t for _, t in sfx) if sfx else None,
               sfx_rows=statistics.mean(k for k, _ in sfx) if sfx else None)
    del b
    torch.cuda.empty_cache()
    return out, toks


def kernel_times():
    from groma_amd import ops
    B, H, hd, Lq, p0 = 8, 32, 128, 64, 512
    S = 1024
    g = torch.Generator().manual_seed(0)
    k = torch.randn((B, H, S, hd), generator=g).to(torch.bfloat16).cuda()
    vt = torch.randn((B, H, hd, S), generator=g).to(torch.bfloat16).cuda()
    per = S // 64
    perm = (torch.randperm(B * per, generator=g) + 1).view(B, per).to(torch.int32).cuda()
    kp = torch.zeros((B * per + 1, H, 64, hd), dtype=torch.bfloat16, device="cuda")
    vp = torch.zeros((B * per + 1, H, hd, 64), dtype=torch.bfloat16, device="cuda")
    for b in range(B):
        for j in range(per):
            kp[int(perm[b, j])] = k[b, :, 64 * j:64 * (j + 1)]
            vp[int(perm[b, j])] = vt[b, :, :, 64 * j:64 * (j + 1)]
    qkv = torch.randn((B * Lq, 3 * H * hd), generator=g).to(torch.bfloat16).cuda()
    cs = torch.randn((S, hd // 2), generator=g).cuda()
    pos = torch.full((B,), p0, dtype=torch.int32, device="cuda")
    slot = lambda: ops.attention(qkv, k, vt, Skv=S, causal=True, pos_dev=pos, pos_stride=1,
                                 fused=dict(B=B, H=H, Lq=Lq, hd=hd, cos=cs, sin=cs))
    paged = lambda: ops.attention_paged(qkv, kp, vp, perm, B=B, H=H, Lq=Lq, hd=hd, pos_dev=pos, pos_stride=1, cos=cs, sin=cs,
                                        fused=True)
    assert torch.equal(slot(), paged())
    out = {}
    for name, fn in (("gr_attention_bf16", slot), ("gr_attention_paged", paged)) * 2:
        for _ in range(5):
            fn()
        ts = []
        for _ in range(50):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        out.setdefault(name, []).append(statistics.median(ts))
    return {k_: min(v) for k_, v in out.items()}


def main():
    reps = int(arg("--reps", 2))
    pages = int(arg("--pages", 768))
    cfg, m = model7b()
    reqs = traffic(cfg, m)
    L = [int(ids.numel()) for ids, _, _ in reqs]
    print(f"Groma-7B width, {len(m.llm.w['layers'])} layers, bf16, synthetic weights; {len(reqs)} requests (8 images x 7 queries, "
          f"un-expanded prompt {min(L)}..{max(L)} ids), kv_pages {pages}, max_len 1024, overlap_admission default (on); {reps} rounds, "
          "cache off / on alternated", flush=True)
    for new in (3, 32):
        for rows in (8, 32):
            res = {False: [], True: []}
            for _ in range(reps):
                for cache in (False, True):
                    out, toks = serve(m, reqs, rows, new, pages, cache)
                    res[cache].append((out, toks))
            same = all(t == res[False][0][1] for _, t in res[True] + res[False])
            for cache in (False, True):
                o = [x for x, _ in res[cache]]
                rps = statistics.median(x["rps"] for x in o)
                adm = statistics.median(x["adm_ms"] for x in o)
                line = (f"new {new:>2} rows {rows:>2} cache {'on ' if cache else 'off'}: {rps:6.1f} req/s (runs "
                        + " ".join(f"{x['rps']:.1f}" for x in o) + f"), admission {adm:5.2f} ms/request, {o[0]['waves']} waves")
                if cache:
                    line += f", hits {o[0]['hits']}, suffix prefill {statistics.median(x['sfx_ms'] for x in o):.2f} ms/wave " \
                            f"({o[0]['sfx_rows']:.1f} rows/wave)"
                print(line, flush=True)
            print(f"new {new:>2} rows {rows:>2}: tokens equal on / off: {same}", flush=True)
    kt = kernel_times()
    print("kernel, 8 rows x 32 heads x 128, 64 queries at 512 (keys 0..575), in-place q + RoPE, median of 50 (best of 2 rounds): "
          + ", ".join(f"{k_} {v:.1f} us" for k_, v in kt.items()), flush=True)


if __name__ == "__main__":
    main()
