"""Paged KV cache (ContinuousBatcher(kv_pages=N), engine.PagedKVCache) on the GPU.

Every comparison is torch.equal: the paged kernels do the slot kernels' arithmetic on the same values, only the addresses differ.
  1. gr_decode_attention_paged == gr_decode_attention (keys scattered over a random page permutation, the sink page NaN);
  2. the paged K / V^T writes (QKV stream, 16-bit and e4m3 weights; gr_qkv_split_paged) == the slot writes, and nothing else moves;
  3. gr_kv_scatter_pages == a torch gather of the staging rows;
  4. a paged batcher's tokens == a slot batcher's (fused / wide / e4m3 / hybrid / eager / overlapped admission / page reuse);
  5. a pool smaller than max_rows x max_len serves a long request among short ones; what does not fit waits, what never fits fails."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _paged_copy(k, vt, lens, gen, sink=float("nan")):
    """slot caches k [B,H,S,hd] / vt [B,H,hd,S] -> pools [P+1,H,64,hd] / [P+1,H,hd,64] over a random page permutation + the table"""
    B, H, S, hd = k.shape
    need = [-(-int(n) // 64) for n in lens]
    P = sum(need)
    perm = (torch.randperm(P, generator=gen) + 1).tolist()
    table = torch.zeros((B, S // 64), dtype=torch.int32)
    kp = torch.full((P + 1, H, 64, hd), sink, dtype=k.dtype, device=k.device)
    vp = torch.full((P + 1, H, hd, 64), sink, dtype=k.dtype, device=k.device)
    i = 0
    for b in range(B):
        for j in range(need[b]):
            pg = perm[i]
            i += 1
            table[b, j] = pg
            kp[pg] = k[b, :, j * 64:(j + 1) * 64]
            vp[pg] = vt[b, :, :, j * 64:(j + 1) * 64]
    return kp, vp, table.to(k.device)


CASES = [(1, (8191,)), (1, (1,)), (4, (1, 63, 64, 65)), (8, (65, 4095, 1, 64, 63, 8191, 200, 130)),
         (16, (1, 63, 64, 65, 4095, 8191)), (64, (1, 63, 64, 65, 4095, 8191, 640, 129))]


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("B,lens", CASES)
def test_decode_attention_paged_equals_slot(hd, B, lens):
    from groma_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + hd)
    H = 512 // hd
    lens = [lens[i % len(lens)] for i in range(B)]
    S = -(-max(lens) // 64) * 64
    k = torch.randn((B, H, S, hd), generator=gen).to(BF).cuda()
    vt = torch.randn((B, H, hd, S), generator=gen).to(BF).cuda()
    # stale bytes beyond each row's length (the kernels must never let them into the result)
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        vt[b, :, :, n:] = float("nan")
    q = torch.randn((B, H, 1, hd), generator=gen).to(BF).cuda()
    kp, vp, table = _paged_copy(k, vt, lens, gen)
    pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device="cuda")
    for nsplit in (1, 3):
        want = torch.zeros((B, H * hd), dtype=BF, device="cuda")
        got = torch.zeros_like(want)
        a = ops.decode_attention(q, k, vt, want, Smax=S, pos_dev=pos, pos_stride=1, nsplit=nsplit)
        a = a[0].clone() if isinstance(a, tuple) else a
        b_ = ops.decode_attention_paged(q, kp, vp, got, table, Smax=S, pos_dev=pos, pos_stride=1, nsplit=nsplit)
        b_ = b_[0].clone() if isinstance(b_, tuple) else b_
        torch.cuda.synchronize()
        if nsplit == 1:
            assert not torch.isnan(want.float()).any()
            assert torch.equal(want, got), (hd, B, nsplit)
        else:
            assert torch.equal(a, b_), (hd, B, nsplit)    # the key-slice parts the o-proj merges
    # a host position (q_pos0) and kv_len give the same bits too
    if B == 4:
        kvl = torch.tensor([max(1, n - 1) for n in lens], dtype=torch.int32, device="cuda")
        want = torch.zeros((B, H * hd), dtype=BF, device="cuda")
        got = torch.zeros_like(want)
        ops.decode_attention(q, k, vt, want, Smax=S, pos_dev=pos, pos_stride=1, kv_len=kvl, nsplit=1)
        ops.decode_attention_paged(q, kp, vp, got, table, Smax=S, pos_dev=pos, pos_stride=1, kv_len=kvl, nsplit=1)
        assert torch.equal(want, got)
        want.zero_(), got.zero_()
        ops.decode_attention(q[:1], k[:1], vt[:1], want[:1], Smax=S, q_pos0=0, nsplit=1)
        ops.decode_attention_paged(q[:1], kp, vp, got[:1], table, Smax=S, q_pos0=0, nsplit=1)
        assert torch.equal(want, got)


def _expect_pools(kp0, vp0, kc, vc, table, pos):
    """the pools as they must look after one write at pos[m] per row: the slot caches' new K row / V^T column, nothing else"""
    kp, vp = kp0.clone(), vp0.clone()
    for m, p in enumerate(pos.tolist()):
        pg = int(table[m, p // 64])
        kp[pg, :, p % 64] = kc[m, :, p]
        vp[pg, :, :, p % 64] = vc[m, :, :, p]
    return kp, vp


def _kv_setup(M, H, hd, S, pos_list, gen):
    sent = 3.0
    kc = torch.full((M, H, S, hd), sent, dtype=BF, device="cuda")
    vc = torch.full((M, H, hd, S), sent, dtype=BF, device="cuda")
    P = M * (S // 64)
    perm = (torch.randperm(P, generator=gen) + 1).view(M, S // 64).to(torch.int32).cuda()
    kp = torch.full((P + 1, H, 64, hd), sent, dtype=BF, device="cuda")
    vp = torch.full((P + 1, H, hd, 64), sent, dtype=BF, device="cuda")
    pos = torch.tensor(pos_list, dtype=torch.int32, device="cuda")
    return kc, vc, kp, vp, perm, pos


@pytest.mark.parametrize("w8", [False, True])
@pytest.mark.parametrize("M", [3, 8])
def test_paged_qkv_stream_writes_equal_slot_writes(w8, M):
    from groma_amd import ops
    gen = torch.Generator().manual_seed(7 + M + 100 * w8)
    H, hd, K, S = 4, 128, 512, 1024
    N = 3 * H * hd
    if w8:
        W = (torch.randn((N, K), generator=gen) * 8).clamp(-448, 448).to(ops.FP8).cuda()
        wsc = (torch.rand((N,), generator=gen) * 0.01 + 0.001).cuda()
        extra = dict(w_scale=wsc)
    else:
        W = (torch.randn((N, K), generator=gen) * 0.05).to(BF).cuda()
        extra = {}
    h = torch.randn((M, K), generator=gen).cuda()
    gamma = (torch.rand((K,), generator=gen) + 0.5).cuda()
    cos = torch.randn((S, hd // 2), generator=gen).cuda()
    sin = torch.randn((S, hd // 2), generator=gen).cuda()
    pos_list = [0, 63, 64, 1023, 200, 5, 130, 999][:M]
    kc, vc, kp, vp, table, pos = _kv_setup(M, H, hd, S, pos_list, gen)
    kp0, vp0 = kp.clone(), vp.clone()
    q1 = torch.zeros((M, H, 1, hd), dtype=BF, device="cuda")
    q2 = torch.zeros_like(q1)
    base = dict(cos=cos, sin=sin, H=H, hd=hd, pos_dev=pos, pos_stride=1)
    ops.gemv_fused(W, M=M, norm=(h, gamma, 1e-5), qkv=dict(q=q1, k=kc, vt=vc, **base), **extra)
    ops.gemv_fused(W, M=M, norm=(h, gamma, 1e-5), qkv=dict(q=q2, k=kp, vt=vp, table=table, **base), **extra)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2)
    ek, ev = _expect_pools(kp0, vp0, kc, vc, table, pos)
    assert torch.equal(kp, ek) and torch.equal(vp, ev)
    assert not torch.equal(kp, kp0) and not torch.equal(vp, vp0)


@pytest.mark.parametrize("B", [16, 64])
def test_paged_qkv_split_writes_equal_slot_writes(B):
    from groma_amd import ops
    gen = torch.Generator().manual_seed(11 + B)
    H, hd, S = 4, 128, 512
    qkv = torch.randn((B, 3 * H * hd), generator=gen).to(BF).cuda()
    cos = torch.randn((S, hd // 2), generator=gen).cuda()
    sin = torch.randn((S, hd // 2), generator=gen).cuda()
    pos_list = [(37 * b + 5 * (b % 3)) % S for b in range(B)]
    kc, vc, kp, vp, table, pos = _kv_setup(B, H, hd, S, pos_list, gen)
    kp0, vp0 = kp.clone(), vp.clone()
    q1 = torch.zeros((B, H, 1, hd), dtype=BF, device="cuda")
    q2 = torch.zeros_like(q1)
    ops.qkv_split(qkv, q1, kc, vc, B=B, H=H, L=1, hd=hd, cos=cos, sin=sin, pos_dev=pos, pos_stride=1)
    ops.qkv_split_paged(qkv, q2, kp, vp, table, B=B, H=H, hd=hd, cos=cos, sin=sin, pos_dev=pos, pos_stride=1)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2)
    ek, ev = _expect_pools(kp0, vp0, kc, vc, table, pos)
    assert torch.equal(kp, ek) and torch.equal(vp, ev)


def test_kv_scatter_pages_equals_a_gather():
    from groma_amd import ops
    gen = torch.Generator().manual_seed(3)
    n_src, H, S, hd, rows, ld = 4, 4, 512, 128, 6, 16
    ks = torch.randn((n_src, H, S, hd), generator=gen).to(BF).cuda()
    vs = torch.randn((n_src, H, hd, S), generator=gen).to(BF).cuda()
    P = 40
    kp = torch.full((P + 1, H, 64, hd), 5.0, dtype=BF, device="cuda")
    vp = torch.full((P + 1, H, hd, 64), 5.0, dtype=BF, device="cuda")
    kp0, vp0 = kp.clone(), vp.clone()
    table = torch.zeros((rows, ld), dtype=torch.int32)
    src, dst, lens = [0, 2, 3], [5, 1, 3], [1, 130, 512]
    perm = (torch.randperm(P, generator=gen) + 1).tolist()
    for d, n in zip(dst, lens):
        for j in range(-(-n // 64)):
            table[d, j] = perm.pop()
    table = table.cuda()
    meta = torch.tensor([src, dst, lens], dtype=torch.int32, device="cuda")
    ops.kv_scatter_pages(ks, vs, kp, vp, table, meta, max(lens))
    torch.cuda.synchronize()
    ek, ev = kp0.clone(), vp0.clone()
    for s, d, n in zip(src, dst, lens):
        for j in range(-(-n // 64)):
            pg = int(table[d, j])
            ek[pg] = ks[s, :, j * 64:(j + 1) * 64]
            ev[pg] = vs[s, :, :, j * 64:(j + 1) * 64]
    assert torch.equal(kp, ek) and torch.equal(vp, ev)


# ------------------------------------------------------------------------------------------------ the batcher
@pytest.fixture(scope="module")
def setup(dev):
    from groma_amd import synth
    cfg, sd, tk = util.tiny_setup(seed=0)
    model = util.device_model(cfg, sd)
    model.generation_config.eos_token_id = None
    reqs = []
    for i in range(6):
        images, ids = synth.make_inputs(cfg, tk, bs=1, seed=300 + i)
        reqs.append((ids[0], images[0], 5 + 4 * i, 700 + i))
    return cfg, sd, model, reqs


def _serve(model, reqs, **kw):
    from groma_amd.serving import ContinuousBatcher
    b = ContinuousBatcher(model, **kw)
    rids = [b.submit(ids, img, max_new_tokens=n, seed=s) for ids, img, n, s in reqs]
    res = b.run_until_done()
    out = []
    for rid in rids:
        assert res[rid].error is None and res[rid].done, res[rid].error
        out.append(res[rid].tokens)
    return b, out


def _solo(model, ids, image, n, seed):
    torch.manual_seed(seed)
    out = model.generate(ids[None].clone(), images=image[None], max_new_tokens=n)
    return out[0, ids.shape[0]:].tolist()


@pytest.mark.parametrize("rows,use_graph,overlap", [(2, True, None), (4, False, False), (8, True, False), (16, True, None)])
def test_paged_batcher_tokens_equal_slot_batcher(setup, rows, use_graph, overlap):
    cfg, sd, model, reqs = setup
    kw = dict(max_rows=rows, max_len=1024, use_graph=use_graph, overlap_admission=overlap)
    _, want = _serve(model, reqs, **kw)
    # 24 pages: at most two requests' bounds (~10 pages each) at a time, so later rows reuse the pages of finished ones
    b, got = _serve(model, reqs, kv_pages=24, **kw)
    assert got == want
    st = b.kv_stats()
    assert st["pages_free"] == st["pages_total"] == 24 and 0 < st["high_water"] <= 24
    assert int(b.arena.table.abs().sum()) == 0          # every row's entries point at the sink page again
    # staging: admit_rows (min(rows, 8)) x max_prompt_len (1024) positions, K and V^T of 2 layers x 4 heads x 128 dims
    assert st["staging_bytes"] == 2 * 2 * min(rows, 8) * 4 * 1024 * 128 * 2
    assert st["pool_bytes"] == 2 * 2 * 25 * 4 * 64 * 128 * 2 + rows * 16 * 4


def test_paged_batcher_over_e4m3_and_hybrid_models(setup):
    from groma_amd import constants
    from groma_amd.groma import GromaModel
    cfg, sd, model, reqs = setup
    for kw in (dict(fp8=True), dict(precision="hybrid")):
        cfg0, sd0, _ = util.tiny_setup(seed=0)
        m = GromaModel.from_state_dict(cfg0, sd0, "cuda", **kw)
        m.init_special_token_id(constants.SyntheticTokenizer())
        m.generation_config.eos_token_id = None
        _, want = _serve(m, reqs[:4], max_rows=2, max_len=1024)
        b, got = _serve(m, reqs[:4], max_rows=2, max_len=1024, kv_pages=64)
        assert got == want, kw
        assert b.pages.n_free == 64


def test_paged_pool_smaller_than_the_slots_serves_a_long_request(setup):
    from groma_amd.serving import ContinuousBatcher
    cfg, sd, model, reqs = setup
    assert cfg.llm_cfg.max_position_embeddings == 4096
    kv_pages = 40                                        # 2560 positions; slots would need 4 x 4096 / 64 = 256 pages
    b = ContinuousBatcher(model, max_rows=4, max_len=4096, kv_pages=kv_pages)
    trace = [(reqs[0], 700), (reqs[1], 12), (reqs[2], 9), (reqs[3], 2200), (reqs[4], 15), (reqs[5], 6)]
    rids = [b.submit(ids, img, max_new_tokens=n, seed=s) for (ids, img, _, s), n in trace]
    waited = False
    for _ in range(5000):
        if not b.queue and not b.slots.active() and b._job is None:
            break
        b.step()
        if b.queue and b.slots.n_free > 0 and b._job is None and b.pages.n_free < -(-b._bound(b.queue[0]) // 64):
            waited = True                                # a row is free, but the head request's pages are not: it waits
        assert b.pages.n_free >= 0 and b.pages.high_water <= kv_pages
    res = {rid: b.live[rid] for rid in rids}
    long_rid, huge_rid = rids[0], rids[3]
    assert res[huge_rid].error is not None and "pool" in res[huge_rid].error and not res[huge_rid].tokens
    assert len(res[long_rid].tokens) == 700 and b._bound(res[long_rid]) > 1024
    assert waited
    for rid, ((ids, img, _, s), n) in zip(rids, trace):
        if rid == huge_rid:
            continue
        r = res[rid]
        assert r.error is None and r.prompt_len + n < 4096
        assert r.tokens == _solo(model, ids, img, n, s), rid
    assert b.pages.n_free == kv_pages and b.pages.high_water <= kv_pages


def test_paged_mode_argument_checks(setup):
    from groma_amd import engine
    from groma_amd.serving import ContinuousBatcher
    cfg, sd, model, reqs = setup
    with pytest.raises(ValueError):
        ContinuousBatcher(model, max_rows=2, max_len=1024, kv_pages=16, grow_to=2048)
    with pytest.raises(ValueError):
        ContinuousBatcher(model, max_rows=2, max_len=8192, kv_pages=16)    # beyond the tiny model's 4096 positions
    with pytest.raises(ValueError):
        ContinuousBatcher(model, max_rows=2, max_len=1000, kv_pages=16)
    llm = model.llm
    cache = llm.new_paged_cache(2, 1024, 4, "cuda")
    h = torch.zeros((4, llm.T), device="cuda")
    with pytest.raises(ValueError):
        llm.forward(h, 2, 2, cache)                                          # an L > 1 step never reads a paged cache
    pos = torch.zeros((2,), dtype=torch.int32, device="cuda")
    old = engine.FUSED_DECODE
    try:
        engine.FUSED_DECODE = False                                          # the general kernels would be taken: refused
        with pytest.raises(ValueError):
            llm.forward(h[:2], 2, 1, cache, pos_dev=pos, pos_stride=1)
    finally:
        engine.FUSED_DECODE = old
