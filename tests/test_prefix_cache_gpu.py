"""Prefix cache of the paged continuous batcher (ContinuousBatcher(kv_pages=N, prefix_cache=True)) on the GPU.

Every comparison of values is torch.equal:
  1. gr_attention_paged == gr_attention_bf16 over a slot cache holding the same keys (ragged rows, scrambled and shared pages, in-place
     q + RoPE, kv_len padding; bf16 and fp16 builds);
  2. gr_kv_append_paged writes == gr_qkv_split's slot writes at the same positions, and no other page moves;
  3. a suffix prefill of positions [p0, L) over pages filled by a cold prefix == rows [p0, L) of a full prefill (16-bit: the logits;
     e4m3: the arg-max tokens);
  4. a batcher with the cache == one without it (tokens, pred_boxes), hits skip the vision stages, shared pages are never written;
  5. a pool too small to keep every entry evicts and still serves every request unchanged;
  6. the same over e4m3 and hybrid models."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


def _pools(caches, n_pos, gen, shared=()):
    """slot caches [(k [H,S,hd], vt [H,hd,S])] -> pools [P+1,H,64,hd] / [P+1,H,hd,64] over a random page permutation (the sink page
    NaN) + the table.  shared = [(row, from_row, n_pages)]: row maps the first n_pages pages of from_row (its slot cache must hold the
    same keys there)."""
    B = len(caches)
    H, S, hd = caches[0][0].shape
    need = [-(-int(n) // 64) for n in n_pos]
    P = sum(need)
    perm = (torch.randperm(P, generator=gen) + 1).tolist()
    table = torch.zeros((B, S // 64), dtype=torch.int32)
    dt, dev = caches[0][0].dtype, caches[0][0].device
    kp = torch.full((P + 1, H, 64, hd), float("nan"), dtype=dt, device=dev)
    vp = torch.full((P + 1, H, hd, 64), float("nan"), dtype=dt, device=dev)
    share = {row: (src, n) for row, src, n in shared}
    for b in range(B):
        for j in range(need[b]):
            if b in share and j < share[b][1]:
                table[b, j] = table[share[b][0], j]
                continue
            pg = perm.pop()
            table[b, j] = pg
            kp[pg] = caches[b][0][:, j * 64:(j + 1) * 64]
            vp[pg] = caches[b][1][:, :, j * 64:(j + 1) * 64]
    return kp, vp, table.to(dev)


# (head dim, Lq, per-row q_pos0): on and off page boundaries; row 1 maps row 0's first page(s) whenever both start past page 0
ATT_CASES = [(128, 1, (70,)), (128, 17, (100, 64, 0, 200)), (128, 64, (128, 70, 5, 300)), (128, 130, (192, 70, 1, 63)),
             (64, 17, (3, 128, 77)), (64, 130, (64, 130, 2))]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("hd,Lq,pos0", ATT_CASES)
def test_attention_paged_equals_slot(dev, precision, hd, Lq, pos0):
    from groma_amd import ops
    with ops.precision(precision):
        dt = ops.H16()
        gen = torch.Generator().manual_seed(hd + Lq)
        B, H = len(pos0), 256 // hd
        S = -(-(max(pos0) + Lq) // 64) * 64 + 64
        k = torch.randn((B, H, S, hd), generator=gen).to(dt).cuda()
        vt = torch.randn((B, H, hd, S), generator=gen).to(dt).cuda()
        shared = []
        if B > 1 and min(pos0[:2]) >= 64:                 # row 1 maps row 0's first page(s): same keys there
            n = min(pos0[1], pos0[0] + Lq) // 64
            if n:
                k[1, :, :64 * n] = k[0, :, :64 * n]
                vt[1, :, :, :64 * n] = vt[0, :, :, :64 * n]
                shared.append((1, 0, n))
        kp, vp, table = _pools([(k[b], vt[b]) for b in range(B)], [p + Lq for p in pos0], gen, shared)
        pos = torch.tensor(pos0, dtype=torch.int32, device="cuda")
        kvl = torch.tensor([max(1, p + Lq - 3 * (b % 2)) for b, p in enumerate(pos0)], dtype=torch.int32, device="cuda")
        cos = torch.randn((S, hd // 2), generator=gen).cuda()
        sin = torch.randn((S, hd // 2), generator=gen).cuda()
        q = torch.randn((B, H, Lq, hd), generator=gen).to(dt).cuda()
        qkv = torch.randn((B * Lq, 3 * H * hd), generator=gen).to(dt).cuda()
        for kv_len in (None, kvl):
            want = ops.attention(q, k, vt, Skv=S, causal=True, kv_len=kv_len, pos_dev=pos, pos_stride=1)
            got = ops.attention_paged(q, kp, vp, table, B=B, H=H, Lq=Lq, hd=hd, kv_len=kv_len, pos_dev=pos, pos_stride=1)
            # in-place q (the fused projection rows) + RoPE at each row's positions
            want2 = ops.attention(qkv, k, vt, Skv=S, causal=True, kv_len=kv_len, pos_dev=pos, pos_stride=1,
                                  fused=dict(B=B, H=H, Lq=Lq, hd=hd, cos=cos, sin=sin))
            got2 = ops.attention_paged(qkv, kp, vp, table, B=B, H=H, Lq=Lq, hd=hd, kv_len=kv_len, pos_dev=pos, pos_stride=1,
                                       cos=cos, sin=sin, fused=True)
            torch.cuda.synchronize()
            assert not torch.isnan(want.float()).any() and not torch.isnan(want2.float()).any()
            assert torch.equal(want, got) and torch.equal(want2, got2), (precision, hd, Lq, pos0, kv_len is None)
        # a host position (every row at the same q_pos0)
        p = min(pos0)
        pos_same = torch.full((B,), p, dtype=torch.int32, device="cuda")
        want = ops.attention(q, k, vt, Skv=S, causal=True, pos_dev=pos_same, pos_stride=1)
        kp2, vp2, table2 = _pools([(k[b], vt[b]) for b in range(B)], [p + Lq] * B, gen)
        got = ops.attention_paged(q, kp2, vp2, table2, B=B, H=H, Lq=Lq, hd=hd, q_pos0=p)
        torch.cuda.synchronize()
        assert torch.equal(want, got)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("hd", [128, 64])
def test_kv_append_paged_writes_equal_slot_writes(dev, precision, hd):
    from groma_amd import ops
    with ops.precision(precision):
        dt = ops.H16()
        gen = torch.Generator().manual_seed(5 + hd)
        H, S, Lq = 4, 512, 70
        pos0 = [0, 60, 129, 5, 448]                      # row 4 runs past its table (448 + 70 > 512): those land in the sink page
        B = len(pos0)
        qkv = torch.randn((B * Lq, 3 * H * hd), generator=gen).to(dt).cuda()
        cos = torch.randn((S + 64, hd // 2), generator=gen).cuda()
        sin = torch.randn((S + 64, hd // 2), generator=gen).cuda()
        kc = torch.full((B, H, S + 64, hd), 3.0, dtype=dt, device="cuda")
        vc = torch.full((B, H, hd, S + 64), 3.0, dtype=dt, device="cuda")
        pos = torch.tensor(pos0, dtype=torch.int32, device="cuda")
        ops.qkv_split(qkv, None, kc, vc, B=B, H=H, L=Lq, hd=hd, cos=cos, sin=sin, pos_dev=pos, pos_stride=1)
        P = B * (S // 64) + 3                                # 3 pages in no table
        perm = (torch.randperm(P, generator=gen) + 1)[: B * (S // 64)].view(B, S // 64).to(torch.int32).cuda()
        kp = torch.randn((P + 1, H, 64, hd), generator=gen).to(dt).cuda()
        vp = torch.randn((P + 1, H, hd, 64), generator=gen).to(dt).cuda()
        ek, ev = kp.clone(), vp.clone()
        ops.kv_append_paged(qkv, kp, vp, perm, B=B, H=H, L=Lq, hd=hd, cos=cos, sin=sin, pos_dev=pos, pos_stride=1)
        torch.cuda.synchronize()
        for b, p0 in enumerate(pos0):
            for p in range(p0, min(p0 + Lq, S)):
                pg = int(perm[b, p // 64])
                ek[pg, :, p % 64] = kc[b, :, p]
                ev[pg, :, :, p % 64] = vc[b, :, :, p]
        assert torch.equal(kp[1:], ek[1:]) and torch.equal(vp[1:], ev[1:])   # (page 0: the sink page, written by row 4's tail)


def _model(**kw):
    from groma_amd import constants
    from groma_amd.groma import GromaModel
    cfg, sd, tk = util.tiny_setup(seed=0)
    m = GromaModel.from_state_dict(cfg, sd, "cuda", **kw)
    m.init_special_token_id(constants.SyntheticTokenizer())
    m.generation_config.eos_token_id = None
    return cfg, tk, m


@pytest.mark.parametrize("kw", [dict(), dict(precision="fp16"), dict(fp8=True)])
def test_suffix_prefill_continues_a_full_prefill(dev, kw):
    from groma_amd import engine, ops, synth
    cfg, tk, m = _model(**kw)
    images, ids = synth.make_inputs(cfg, tk, bs=2, seed=41)
    out = m.forward(input_ids=ids.clone(), images=images, use_cache=True, return_dict=True, _seeds=[3, 4], _keep_embeds=True)
    Ls = [int(x) for x in m._last_aux["lengths"]]
    emb = m._last_aux["inputs_embeds"]
    full = out.logits.clone()
    slot = out.past_key_values
    llm = m.llm
    with ops.precision(m.precision):
        for p0s in ((64, 128), (128, 192)):
            n_pages = 2 * (slot.smax // 64) + 2
            cache = llm.new_paged_cache(2, slot.smax, n_pages, "cuda")
            perm = (torch.randperm(n_pages, generator=torch.Generator().manual_seed(p0s[0])) + 1)
            table = perm[: 2 * (slot.smax // 64)].view(2, -1).to(torch.int32).cuda()
            cache.table.copy_(table)
            # the cold prefixes [0, p0_b) of both rows, then the suffixes, padded to a common length
            meta = torch.tensor([[0, 1], [0, 1], list(p0s)], dtype=torch.int32, device="cuda")
            for l in range(len(cache.k)):
                ops.kv_scatter_pages(slot.k[l], slot.vt[l], cache.k[l], cache.vt[l], table, meta, slot.smax)
            Lq = max(L - p for L, p in zip(Ls, p0s))
            h = torch.zeros((2 * Lq, llm.T), device="cuda")
            for b, (L, p) in enumerate(zip(Ls, p0s)):
                h[b * Lq: b * Lq + L - p] = emb[b, p:L]
            pos = torch.tensor(p0s, dtype=torch.int32, device="cuda")
            kvl = torch.tensor(Ls, dtype=torch.int32, device="cuda")
            adm = torch.zeros((2, slot.smax // 64), dtype=torch.int32, device="cuda")
            adm.copy_(table)
            got = llm.prefill_paged(h, 2, Lq, cache, adm, pos, kvl)
            torch.cuda.synchronize()
            for b, (L, p) in enumerate(zip(Ls, p0s)):
                g, w = got[b, : L - p], full[b, p:L]
                if kw.get("fp8"):
                    assert torch.equal(g.argmax(-1), w.argmax(-1)), (kw, b, p)
                else:
                    assert torch.equal(g, w), (kw, b, p, (g - w).abs().max().item())
    assert isinstance(cache, engine.PagedKVCache)


# ------------------------------------------------------------------------------------------------ the batcher
def _traffic(cfg, tk, n_img=3, n_q=4):
    """n_img images x n_q queries: each query keeps its image's prompt head (through <region> and a few ids) and ends differently"""
    from groma_amd import synth
    out = []
    for i in range(n_img):
        images, ids = synth.make_inputs(cfg, tk, bs=1, seed=900 + i)
        head = ids[0][:40]
        g = torch.Generator().manual_seed(50 + i)
        for j in range(n_q):
            tail = torch.randint(3, cfg.llm_cfg.vocab_size, (20 + 7 * j,), generator=g)
            out.append((torch.cat([head, tail]), images[0], 3 if j % 2 == 0 else 9, 700 + i))
    return out


def _run(model, reqs, first=None, **kw):
    """serve `reqs`; with `first`, those requests go in first and the rest only once they are placed (so that they can hit)"""
    from groma_amd.serving import ContinuousBatcher
    b = ContinuousBatcher(model, **kw)
    order = list(range(len(reqs)))
    head = order if first is None else first
    rids = {}
    for i in head:
        ids, img, n, s = reqs[i]
        rids[i] = b.submit(ids, img, max_new_tokens=n, seed=s)
    if first is not None:
        for _ in range(1000):
            if all(b.live[rids[i]].tokens or b.live[rids[i]].done for i in head) and b._job is None:
                break
            b.step()
        for i in order:
            if i not in rids:
                ids, img, n, s = reqs[i]
                rids[i] = b.submit(ids, img, max_new_tokens=n, seed=s)
    res = b.run_until_done()
    out = []
    for i in order:
        r = res[rids[i]]
        assert r.error is None and r.done, r.error
        out.append((r.tokens, r.pred_boxes.cpu()))
    return b, out


def _same(got, want):
    assert [t for t, _ in got] == [t for t, _ in want]
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(got, want))


@pytest.fixture(scope="module")
def served(dev):
    cfg, tk, m = _model()
    reqs = _traffic(cfg, tk)
    _, want = _run(m, reqs, max_rows=4, max_len=1024, kv_pages=64)
    return cfg, tk, m, reqs, want


@pytest.mark.parametrize("use_graph,overlap", [(True, None), (True, False), (False, False)])
def test_batcher_with_prefix_cache_equals_without(served, use_graph, overlap):
    cfg, tk, m, reqs, want = served
    calls = []
    fwd = m.forward

    def counting(*a, **kw):
        calls.append(int(kw["input_ids"].shape[0]))
        return fwd(*a, **kw)
    m.forward = counting
    try:
        firsts = [0, 4, 8]
        b, got = _run(m, reqs, first=firsts, max_rows=4, max_len=1024, kv_pages=64, prefix_cache=True, use_graph=use_graph,
                      overlap_admission=overlap)
    finally:
        del m.forward
    _same(got, want)
    st = b.kv_stats()
    assert st["prefix_hits"] == 9 and st["prefix_misses"] == 3 and st["prefix_entries"] == 3
    assert sum(calls) == 3                                # the vision stages and the full prefill ran for the cold requests only
    # the entries' pages hold the cold prompts' KV: never written by a hit, whatever ran since
    pages = sorted({p for e in b.prefix.entries.values() for p in e.pages})
    snap = [(t[pages].clone(), u[pages].clone()) for t, u in zip(b.arena.k, b.arena.vt)]
    assert st["pages_shared"] == 0 and st["pages_free"] == 64 - len(pages)
    # a different seed, a different image, no seed: misses
    ids, img, n, s = reqs[1]
    other = _traffic(cfg, tk, n_img=4, n_q=1)[3]
    for ids_, img_, seed in ((ids, img, s + 1), (other[0], other[1], s), (ids, img, None)):
        rid = b.submit(ids_, img_, max_new_tokens=3, seed=seed)
        b.run_until_done()
        assert b.live[rid].error is None and len(b.live[rid].tokens) == 3
    st = b.kv_stats()
    assert st["prefix_hits"] == 9 and st["prefix_misses"] == 6 and st["prefix_entries"] == 5
    for (k0, v0), t, u in zip(snap, b.arena.k, b.arena.vt):
        assert torch.equal(k0, t[pages]) and torch.equal(v0, u[pages])
    b.clear_prefix_cache()
    st = b.kv_stats()
    assert st["prefix_entries"] == 0 and st["pages_free"] == st["pages_total"] == 64 and st["pages_shared"] == 0
    assert int(b.arena.table.abs().sum()) == 0


def test_prefix_cache_evicts_when_the_pool_is_small(served):
    from groma_amd.serving import ContinuousBatcher, Request
    cfg, tk, m, reqs, want = served
    probe = ContinuousBatcher(m, max_rows=2, max_len=1024, kv_pages=64)
    need = max(-(-probe._bound(Request(0, ids, img, n)) // 64) for ids, img, n, _ in reqs)
    del probe
    # room for one request's bound and two pages more: a cold request of the next image evicts the entries of earlier ones
    order = [0, 1, 2, 4, 3, 5, 8, 6, 9, 7, 10, 11]
    b, got = _run(m, [reqs[i] for i in order], first=[0], max_rows=2, max_len=1024, kv_pages=need + 2, prefix_cache=True)
    _same(got, [want[i] for i in order])
    assert b.prefix.evicted > 0 and b.kv_stats()["prefix_hits"] > 0
    b.clear_prefix_cache()
    assert b.pages.n_free == need + 2


@pytest.mark.parametrize("kw", [dict(fp8=True), dict(precision="hybrid")])
def test_prefix_cache_over_e4m3_and_hybrid_models(dev, kw):
    cfg, tk, m = _model(**kw)
    reqs = _traffic(cfg, tk, n_img=2, n_q=3)
    _, want = _run(m, reqs, max_rows=4, max_len=1024, kv_pages=64)
    b, got = _run(m, reqs, first=[0, 3], max_rows=4, max_len=1024, kv_pages=64, prefix_cache=True)
    assert [t for t, _ in got] == [t for t, _ in want], kw
    assert b.kv_stats()["prefix_hits"] == 4
    b.clear_prefix_cache()
    assert b.pages.n_free == 64
