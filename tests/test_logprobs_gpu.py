"""Per-token log-probabilities and scores (gr_sample_rows_lp) on the GPU: the kernel against the CPU, generate(), the batcher.

Exact parts are torch.equal.  The log-probabilities are compared with float64 under a bound that is derived, not chosen: the error
a float32 restatement of the kernel's formula (numpy, same summation order) makes against float64 on the same inputs, times 8 for
the device's few-ulp exp / log intrinsics (`_tolerance`)."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

F32 = np.float32


# ------------------------------------------------------------------------------------------------ CPU restatements
def _lp_f32(x):
    """gr_sample_rows_lp's log-softmax of one row in numpy float32, sum in the kernel's order: 1024 contiguous chunks summed in index
    order, a Hillis-Steele scan over the 64 lanes of each wave (lane 63 holds the wave total), the 16 wave totals in order"""
    x = np.asarray(x, dtype=F32)
    V = x.shape[0]
    chunk = (V + 1023) // 1024
    m = x.max()
    e = np.zeros(1024 * chunk, dtype=F32)
    e[:V] = np.exp((x - m).astype(F32)).astype(F32)
    e = e.reshape(1024, chunk)
    local = np.zeros(1024, dtype=F32)
    for j in range(chunk):
        local = (local + e[:, j]).astype(F32)
    incl = local.reshape(16, 64).copy()
    o = 1
    while o < 64:
        nxt = incl.copy()
        nxt[:, o:] = (incl[:, o:] + incl[:, :-o]).astype(F32)
        incl, o = nxt, o * 2
    total = F32(0)
    for w in range(16):
        total = F32(total + incl[w, 63])
    return ((x - m).astype(F32) - F32(np.log(total))).astype(F32)


def _cases():
    """(name, x [rows, ld] f32, V): every input row the issue lists; ld > V everywhere"""
    g = torch.Generator().manual_seed(77)
    out = []
    V = 32128
    x = torch.randn((12, V + 8), generator=g) * 3.0
    # (_row_args: rows 0, 3, 5, 8, 10 are greedy; k = 8 on rows 1, 4, 8, 11)
    x[0, [5, 17000, 32127]] = x[0, :V].max() + 1.0                  # exact ties at the maximum, greedy row: the first index wins
    top = x[8, :V].max()
    x[8, [31000, 40, 900]] = top - 0.5                              # exact ties inside the top 8 (index order: 40, 900, 31000)
    x[8, [20000, 20001]] = top - 0.25
    x[11, [7, 8, 9]] = x[11, :V].max()                              # ties at the maximum on a sampled row, k = 8
    for row in (1, 3):                                              # one dominant logit (sampled / greedy): every other exp underflows to 0
        x[row, :V] = torch.randn((V,), generator=g)
        x[row, 12345] = 200.0
    x[4, :V] = (torch.randn((V,), generator=g) * 2.0).round()       # a row of very few distinct values (ties everywhere)
    x[:, V:] = 1e30                                                 # the padding behind V must never be read as a logit
    out.append(("V32128", x, V))
    for V in (5000, 1000, 37):                                      # not a multiple of 1024; below 1024; fewer logits than waves
        x = torch.randn((6, V + 24), generator=g) * 2.0
        x[0, [V - 1, 3]] = x[0, :V].max() + 2.0
        x[:, V:] = 1e30
        out.append((f"V{V}", x, V))
    return out


def _row_args(rows):
    inv = torch.tensor([(0.0, 1.0 / 0.7, 1.0, 0.0, 2.0)[i % 5] for i in range(rows)])
    k = torch.tensor([(5, 8, 0, 1, 8, 5, 1)[i % 7] for i in range(rows)], dtype=torch.int32)
    seeds = torch.arange(rows, dtype=torch.int64) * 7919 + 13
    pos = torch.arange(rows, dtype=torch.int32) * 3 + 20
    return inv, k, seeds, pos


def _run_kernel(x, V, step=1, steps=3):
    from groma_amd import ops
    rows = x.shape[0]
    inv, k, seeds, pos = _row_args(rows)
    xd = x.cuda()
    a = dict(pos=pos.cuda(), pos_stride=1, pos_off=1)
    want_tok = ops.sample_rows(xd, V, inv.cuda(), seeds.cuda(), **a)
    top_ids = torch.full((rows, 8), -7, dtype=torch.int64, device="cuda")
    top_lp = torch.full((rows, 8), 7.0, device="cuda")
    scores = torch.full((steps, rows, V), 5.0, device="cuda")
    st = torch.tensor([step], dtype=torch.int32, device="cuda")
    tok, lp = ops.sample_rows_lp(xd, V, inv.cuda(), seeds.cuda(), k=k.cuda(), top_ids=top_ids, top_lp=top_lp, scores=scores, step=st, **a)
    torch.cuda.synchronize()
    return dict(inv=inv, k=k, want_tok=want_tok.cpu(), tok=tok.cpu(), lp=lp.cpu(), top_ids=top_ids.cpu(), top_lp=top_lp.cpu(),
                scores=scores.cpu())


def _tolerance(cases, picks):
    """(8 x e, e): e = the largest error of the float32 restatement against float64 over every compared entry (the chosen token and
    the k best of every row of every case).  picks[name] = [(row, [ids])]."""
    e = 0.0
    for name, x, V in cases:
        for row, ids in picks[name]:
            ref = torch.log_softmax(x[row, :V].double(), -1)
            got = torch.from_numpy(_lp_f32(x[row, :V].numpy())).double()
            e = max(e, float((got[ids] - ref[ids]).abs().max()))
    return 8.0 * e, e


_MEASURED = {}


def _measure():
    """the module's one measurement: runs the kernel on every row of _cases() and returns (bound, float32 error, device error)"""
    if not _MEASURED:
        cases = _cases()
        runs = {name: _run_kernel(x, V) for name, x, V in cases}
        picks = {}
        for name, x, V in cases:
            r = runs[name]
            picks[name] = [(row, [int(r["tok"][row])] + r["top_ids"][row, : min(int(r["k"][row]), V)].tolist()) for row in range(x.shape[0])]
        tol, e32 = _tolerance(cases, picks)
        worst = 0.0
        for name, x, V in cases:
            r = runs[name]
            for row, ids in picks[name]:                              # every row: nothing skipped or filtered
                ref = torch.log_softmax(x[row, :V].double(), -1)
                got = torch.cat([r["lp"][row: row + 1], r["top_lp"][row, : len(ids) - 1]]).double()
                worst = max(worst, float((got - ref[ids]).abs().max()))
        _MEASURED.update(tol=tol, e32=e32, dev=worst)
    return _MEASURED["tol"], _MEASURED["e32"], _MEASURED["dev"]


# ------------------------------------------------------------------------------------------------ the kernel
def test_kernel_exact_parts(dev):
    """tokens == gr_sample_rows; top-k ids == a stable sort by (value descending, index ascending); the scores slot == the raw row
    (greedy) / the fp32 product x * inv_temp (sampled); a step at capacity writes nothing; two calls give the same bits"""
    for name, x, V in _cases():
        r = _run_kernel(x, V)
        assert torch.equal(r["tok"], r["want_tok"]), name
        for row in range(x.shape[0]):
            k = int(r["k"][row])
            order = torch.sort(x[row, :V], descending=True, stable=True).indices
            kk = min(k, V)
            assert torch.equal(r["top_ids"][row, :kk], order[:kk]), (name, row)
            assert bool((r["top_ids"][row, kk:] == -1).all()) and bool(torch.isinf(r["top_lp"][row, kk:]).all()), (name, row)
            if float(r["inv"][row]) == 0.0:
                assert int(r["tok"][row]) == int(order[0]), (name, row)
                assert torch.equal(r["scores"][1, row], x[row, :V]), (name, row)
            else:
                assert torch.equal(r["scores"][1, row], x[row, :V] * r["inv"][row]), (name, row)
        assert bool((r["scores"][0] == 5.0).all()) and bool((r["scores"][2] == 5.0).all()), name      # the other slots: untouched
        again = _run_kernel(x, V)
        for key in ("tok", "lp", "top_ids", "top_lp", "scores"):
            assert torch.equal(r[key].view(torch.int32) if r[key].dtype == torch.float32 else r[key],
                               again[key].view(torch.int32) if again[key].dtype == torch.float32 else again[key]), (name, key)
        full = _run_kernel(x, V, step=3)                                                              # a step at capacity
        assert bool((full["scores"] == 5.0).all()) and torch.equal(full["tok"], r["tok"]), name
        assert torch.equal(full["lp"].view(torch.int32), r["lp"].view(torch.int32)), name             # (lp_steps = 0: always written)
    assert int(x.shape[0]) > 0


def test_kernel_step_indexed_arenas_and_token_only_rows(dev):
    """logprob [rows, steps] / top_* [rows, steps, kmax] are written at the device step and nowhere else; a step beyond them writes
    nothing; k[row] < 0 rows give their token and leave every output of the row alone"""
    from groma_amd import ops
    name, x, V = _cases()[1]
    rows = x.shape[0]
    inv, k, seeds, pos = _row_args(rows)
    k[2] = -1
    k[3] = -1                                                        # one sampled, one greedy row that do not ask
    flat = _run_kernel(x, V)
    for step in (2, 4):
        lp = torch.full((rows, 4), 9.0, device="cuda")
        top_ids = torch.full((rows, 4, 8), -7, dtype=torch.int64, device="cuda")
        top_lp = torch.full((rows, 4, 8), 7.0, device="cuda")
        st = torch.tensor([step], dtype=torch.int32, device="cuda")
        tok, _ = ops.sample_rows_lp(x.cuda(), V, inv.cuda(), seeds.cuda(), pos=pos.cuda(), pos_stride=1, pos_off=1, k=k.cuda(),
                                    logprob=lp, top_ids=top_ids, top_lp=top_lp, step=st)
        assert torch.equal(tok.cpu(), flat["tok"])
        lp, top_ids, top_lp = lp.cpu(), top_ids.cpu(), top_lp.cpu()
        asks = (k >= 0)
        for s in range(4):
            hit = asks if s == step else torch.zeros_like(asks)
            assert torch.equal(lp[:, s] != 9.0, hit), (step, s)
            assert torch.equal((top_ids[:, s] != -7).all(-1), hit), (step, s)
        if step < 4:
            keep = asks.nonzero().flatten()
            assert torch.equal(lp[keep, step].view(torch.int32), flat["lp"][keep].view(torch.int32))
            kk = [r for r in keep.tolist() if int(k[r]) == int(flat["k"][r])]
            assert torch.equal(top_ids[kk, step], flat["top_ids"][kk])


def test_kernel_logprobs_against_float64(dev):
    """Chosen-token and top-k log-probabilities of EVERY row of the input set against torch.log_softmax in float64.
    Bound = 8 x the float32 restatement's own maximum error on the same entries (_tolerance).
    Measured on an MI355X: float32 restatement 6.914e-06 (the dominant-logit rows: x - m is near -200, where a float32 ulp is
    1.5e-05) -> bound 5.531e-05; device 6.914e-06."""
    tol, e32, worst = _measure()
    print(f"\nlogprob error vs float64: float32 restatement {e32:.3e} -> bound {tol:.3e}; device {worst:.3e}")
    assert e32 > 0.0 and worst <= tol, (worst, tol)


# ------------------------------------------------------------------------------------------------ generate()
@pytest.fixture(scope="module")
def gen(dev):
    from groma_amd import synth
    cfg, sd, tk = util.tiny_setup(seed=0)
    model = util.device_model(cfg, sd)
    model.generation_config.eos_token_id = None
    images, ids = synth.make_inputs(cfg, tk, bs=2, seed=1234)
    return cfg, model, images, ids, _measure()[0]


def _generate(model, ids, images, graph, seed=5, **kw):
    old = model.decode_graph
    model.decode_graph = graph
    try:
        torch.manual_seed(seed)
        return model.generate(ids.clone(), images=images, max_new_tokens=7, **kw)
    finally:
        model.decode_graph = old


@pytest.mark.parametrize("sample", [False, True])
def test_generate_scores_and_logprobs(gen, sample):
    cfg, model, images, ids, tol = gen
    P, n, V = ids.shape[1], 7, cfg.vocab_size
    kw = dict(do_sample=True, temperature=0.9) if sample else {}
    plain = _generate(model, ids, images, True, return_dict_in_generate=True, **kw)
    assert plain.scores is None and plain.logprobs is None and plain.top_ids is None and plain.top_logprobs is None
    outs = {g: _generate(model, ids, images, g, return_dict_in_generate=True, output_scores=True, output_logprobs=5, **kw)
            for g in (True, False)}
    o = outs[True]
    assert torch.equal(o.sequences, plain.sequences)                 # the new outputs change no token
    assert isinstance(o.scores, tuple) and len(o.scores) == n
    assert all(s.shape == (2, V) and s.dtype == torch.float32 for s in o.scores)
    assert o.logprobs.shape == (2, n) and o.top_ids.shape == (2, n, 5) and o.top_logprobs.shape == (2, n, 5)
    for i in range(n):
        tok = o.sequences[:, P + i]
        if not sample:   # greedy: scores are the raw logits (sampled: logits / temperature, while log-probabilities stay those of the raw logits)
            assert torch.equal(o.scores[i].argmax(-1), tok)
            ref = torch.log_softmax(o.scores[i].double(), -1)
            assert float((o.logprobs[:, i].double() - ref.gather(1, tok[:, None])[:, 0]).abs().max()) <= tol
            assert float((o.top_logprobs[:, i].double() - ref.gather(1, o.top_ids[:, i])).abs().max()) <= tol
            assert torch.equal(o.top_ids[:, i], torch.sort(o.scores[i], descending=True, stable=True).indices[:, :5])
    e = outs[False]                                                 # eager loop == captured loop, bit for bit
    assert torch.equal(o.sequences, e.sequences) and torch.equal(o.top_ids, e.top_ids)
    assert torch.equal(o.logprobs.view(torch.int32), e.logprobs.view(torch.int32))
    assert torch.equal(o.top_logprobs.view(torch.int32), e.top_logprobs.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(o.scores, e.scores))
    # each output alone; k = 0 is the chosen token only
    only = _generate(model, ids, images, True, return_dict_in_generate=True, output_logprobs=0, **kw)
    assert only.scores is None and only.top_ids is None and torch.equal(only.logprobs.view(torch.int32), o.logprobs.view(torch.int32))
    sc = _generate(model, ids, images, True, return_dict_in_generate=True, output_scores=True, **kw)
    assert sc.logprobs is None and all(torch.equal(a, b) for a, b in zip(sc.scores, o.scores))


def test_generate_finished_rows_and_argument_check(gen):
    cfg, model, images, ids, tol = gen
    P = ids.shape[1]
    free = _generate(model, ids, images, True, return_dict_in_generate=True, output_logprobs=2)
    eos = int(free.sequences[0, P + 2])                              # row 0 finishes at its third token
    gc = model.generation_config
    old = (gc.eos_token_id, gc.pad_token_id)
    try:
        gc.eos_token_id, gc.pad_token_id = eos, 0
        outs = [_generate(model, ids, images, g, return_dict_in_generate=True, output_logprobs=2, output_scores=True) for g in (True, False)]
    finally:
        gc.eos_token_id, gc.pad_token_id = old
    for o in outs:
        new = o.sequences[:, P:]
        n = new.shape[1]
        assert o.logprobs.shape == (2, n) and len(o.scores) == n
        for b in range(2):
            hit = (new[b] == eos).nonzero().flatten()
            end = int(hit[0]) + 1 if len(hit) else n
            assert torch.equal(o.logprobs[b, :end].view(torch.int32), free.logprobs[b, :end].view(torch.int32))
            assert bool((o.logprobs[b, end:] == 0.0).all()) and bool((new[b, end:] == 0).all())
    assert torch.equal(outs[0].logprobs, outs[1].logprobs) and torch.equal(outs[0].sequences, outs[1].sequences)
    for bad in (9, -1, 1.5):
        with pytest.raises(ValueError):
            model.generate(ids.clone(), images=images, max_new_tokens=2, return_dict_in_generate=True, output_logprobs=bad)


# ------------------------------------------------------------------------------------------------ the batcher
@pytest.fixture(scope="module")
def traffic(dev):
    from groma_amd import constants, synth
    from groma_amd.groma import GromaModel
    cfg, sd, tk = util.tiny_setup(seed=0)
    m = GromaModel.from_state_dict(cfg, sd, "cuda")
    m.init_special_token_id(constants.SyntheticTokenizer())
    m.generation_config.eos_token_id = None
    reqs = []
    for i in range(8):
        images, ids = synth.make_inputs(cfg, tk, bs=1, seed=900 + i)
        g = torch.Generator().manual_seed(50 + i)
        tail = torch.randint(3, cfg.llm_cfg.vocab_size, (20 + 5 * i,), generator=g)
        reqs.append((torch.cat([ids[0][:40], tail]), images[0], 5 + (i % 3) * 3, 700 + i))
    return cfg, m, reqs


def _serve(model, reqs, asks, temps=None, first=None, **kw):
    """serve reqs[i] with logprobs=asks[i]; `first`: those go in alone and the rest once they are placed.  Returns (batcher, results)."""
    from groma_amd.serving import ContinuousBatcher

    class Counting(ContinuousBatcher):       # (a subclass, not a wrapper stored on the instance: no reference cycle through the graphs)
        def _capture(self):
            self.captures.append(1)
            return super()._capture()
    b = Counting(model, **kw)
    b.captures = []
    rids = {}
    order = list(range(len(reqs)))
    for i in (order if first is None else first):
        ids, img, n, s = reqs[i]
        rids[i] = b.submit(ids, img, max_new_tokens=n, seed=s, logprobs=asks[i], temperature=(temps or {}).get(i, 0.0))
    if first is not None:
        for _ in range(1000):
            if all(b.live[rids[i]].tokens or b.live[rids[i]].done for i in first) and b._job is None:
                break
            b.step()
        for i in order:
            if i not in rids:
                ids, img, n, s = reqs[i]
                rids[i] = b.submit(ids, img, max_new_tokens=n, seed=s, logprobs=asks[i], temperature=(temps or {}).get(i, 0.0))
    res = b.run_until_done()
    out = []
    for i in order:
        r = res[rids[i]]
        assert r.error is None and r.done, r.error
        assert (r.logprobs is None) == (asks[i] is None)
        if asks[i] is not None:
            assert len(r.logprobs) == len(r.tokens) == reqs[i][2]
            assert r.top_logprobs is None if asks[i] == 0 else (len(r.top_logprobs) == len(r.tokens) and all(len(t) == asks[i] for t in r.top_logprobs))
        out.append(r)
    return b, out


@pytest.mark.parametrize("mode", ["slots", "paged", "prefix"])
def test_batcher_logprobs_are_a_function_of_the_request(traffic, mode):
    """A request's log-probabilities are bitwise the same solo, beside seven rows of which some do not ask, paged or on slots, cold or
    on a prefix-cache hit; asking changes no token; requests that ask and requests that do not share ONE captured step."""
    cfg, m, reqs = traffic
    kw = {"slots": {}, "paged": dict(kv_pages=96), "prefix": dict(kv_pages=96, prefix_cache=True)}[mode]
    temps = {0: 0.0, 1: 0.8}
    for t in (0, 1):                                                 # a greedy and a sampled target
        tk = {0: temps[t]}
        _, (base,) = _serve(m, [reqs[t]], [5], tk, max_rows=8, max_len=1024)                        # slots, solo: the reference
        _, (quiet,) = _serve(m, [reqs[t]], [None], tk, max_rows=8, max_len=1024, **kw)
        assert quiet.tokens == base.tokens and quiet.logprobs is None
        b, (solo,) = _serve(m, [reqs[t]], [5], tk, max_rows=8, max_len=1024, **kw)
        assert solo.tokens == base.tokens and solo.logprobs == base.logprobs and solo.top_logprobs == base.top_logprobs
        assert len(b.captures) == 1
        # beside seven others: half do not ask, the rest ask for other widths; the target is request 0 of the wave
        others = [reqs[i] for i in range(8) if i != t]
        asks = [5, None, 0, None, 8, None, 1, None]
        b, res = _serve(m, [reqs[t]] + others, asks, tk, max_rows=8, max_len=1024, **kw)
        assert res[0].tokens == base.tokens and res[0].logprobs == base.logprobs and res[0].top_logprobs == base.top_logprobs
        assert len(b.captures) == 1
        if mode == "prefix":                                         # the same request again: a hit, prefilled from p0 on the pool
            b, res = _serve(m, [reqs[t]] * 3, [5, 5, None], {i: temps[t] for i in range(3)}, first=[0], max_rows=8, max_len=1024, **kw)
            assert b.kv_stats()["prefix_hits"] == 2 and b.kv_stats()["prefix_misses"] == 1
            for r in res[:2]:
                assert r.tokens == base.tokens and r.logprobs == base.logprobs and r.top_logprobs == base.top_logprobs
            assert res[2].tokens == base.tokens and len(b.captures) == 1
    # alternating traffic on one batcher: requests that ask and requests that do not never re-capture the step
    b, res = _serve(m, reqs[:6], [3, None, 0, None, 8, None], first=[0, 1], max_rows=2, max_len=1024, **kw)
    assert len(b.captures) == 1 and int(b.lp_k.max()) == -1


def test_batcher_logprobs_equal_generate(traffic):
    """generate(output_logprobs=5) on the same request against a one-row batcher: the decode step of both is the weight-streaming
    path at one row over a slot cache of the same kernels, so the logits -- and with them the log-probabilities -- are the same bits."""
    cfg, m, reqs = traffic
    tol = _measure()[0]
    for t in (0, 3):
        ids, img, n, seed = reqs[t]
        _, (r,) = _serve(m, [reqs[t]], [5], max_rows=1, max_len=1024)
        torch.manual_seed(seed)
        o = m.generate(ids[None].clone(), images=img[None], max_new_tokens=n, return_dict_in_generate=True, output_logprobs=5)
        assert o.sequences[0, ids.shape[0]:].tolist() == r.tokens
        got = torch.tensor(r.logprobs, dtype=torch.float64)
        err = float((got - o.logprobs[0].cpu().double()).abs().max())
        top = torch.tensor([[lp for _, lp in tl] for tl in r.top_logprobs], dtype=torch.float64)
        err = max(err, float((top - o.top_logprobs[0].cpu().double()).abs().max()))
        same = got.float().tolist() == o.logprobs[0].cpu().tolist()
        print(f"\nbatcher vs generate, request {t}: max |diff| {err:.3e}, bitwise {'equal' if same else 'different'}")
        assert err <= tol
        assert [[i for i, _ in tl] for tl in r.top_logprobs] == o.top_ids[0].cpu().tolist()
