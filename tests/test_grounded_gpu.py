"""Grounded decoding on the GPU: gr_grammar_step against this file's own restatement of the grammar table (exact), the sampler behind
the mask (float64 inverse CDF over the allowed ids), generate(grounded=True) and ContinuousBatcher(grounded=True) on the tiny
synthetic model whose output head is scaled until an unconstrained answer breaks the grammar.

The restatement below is this file's own (vectorised for the kernel test); nothing is imported from groma_amd.grammar to decide
what is right."""
import types

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64


# ------------------------------------------------------------------------------------------------ the restatement
def _G(V, bor, eor, r0, rc, never):
    return types.SimpleNamespace(V=V, bor=bor, eor=eor, r0=r0, rc=rc, never=tuple(never))


def _next(g, s, t):
    if s < 0 or t is None:
        return s
    return 1 if t == g.bor else 2 if g.r0 <= t < g.r0 + g.rc else 0 if t == g.eor else s


def _banned(g, s, n):
    """bool [V]"""
    n = max(0, min(n, g.rc))
    m = torch.zeros(g.V, dtype=torch.bool)
    if s < 0:
        return m
    if s == 0:
        m[g.r0: g.r0 + g.rc] = True
        m[[g.eor] + list(g.never) + ([g.bor] if n == 0 else [])] = True
        return m
    m[:] = True
    m[g.r0: g.r0 + n] = False
    if s == 2 or n == 0:
        m[g.eor] = False
    return m


def _states(g, new):
    """the state in front of every token of `new`, from TEXT"""
    out, s = [], 0
    for t in new:
        out.append(s)
        s = _next(g, s, int(t))
    return out, s


def _violation(g, new, n, eos):
    """index of the first banned token, or None; what follows the first EOS is padding"""
    s = 0
    for i, t in enumerate(int(x) for x in new):
        if bool(_banned(g, s, n)[t]):
            return i
        if t == eos:
            return None
        s = _next(g, s, t)
    return None


def _gids(g):
    from groma_amd.grammar import GrammarIds
    return GrammarIds(g.bor, g.eor, g.r0, g.rc, g.never)


# ------------------------------------------------------------------------------------------------ 1. the kernel, exact
@pytest.mark.parametrize("shape", ["V32114", "V300"])
def test_kernel_is_the_table_bit_for_bit(dev, shape):
    """every (state, last token, n): row == where(banned, -inf, input) bit for bit, columns V..ld and state -1 rows unchanged, the
    stored state == the restatement's"""
    from groma_amd import ops
    if shape == "V32114":
        g, ld = _G(32114, 32004, 32005, 32014, 100, (32008, 32009, 32010, 32011, 32012, 32000)), 32128
    else:   # one element per lane; R straddles the wave boundaries at 192 and 256
        g, ld = _G(300, 8, 9, 150, 100, (10, 11, 12, 299)), 320
    ids = _gids(g)
    ns = (0, 1, 37, 100)
    gen = torch.Generator().manual_seed(3)
    for with_tok in (False, True):
        rows = []
        for s in (-1, 0, 1, 2):
            for n in ns:
                toks = [None] if not with_tok else [g.bor, g.eor, g.r0, g.r0 + g.rc - 1, g.r0 + min(n, g.rc - 1), 17, g.never[0]]
                rows += [(s, t, n) for t in toks]
        R = len(rows)
        x = torch.randn((R, ld), generator=gen) * 4.0
        x[:, g.V:] = 1e30
        x[0, 5] = float("-inf")                                             # (a -inf of the input's own stays what it is)
        state = torch.tensor([r[0] for r in rows], dtype=I32)
        n_b = torch.tensor([r[2] for r in rows], dtype=I32)
        tok = torch.tensor([r[1] for r in rows], dtype=I64).to(dev) if with_tok else None
        xd, sd = x.to(dev), state.to(dev)
        back = ops.grammar_step(xd, g.V, sd, n_b.to(dev), ids, last_tok=tok)
        assert back is xd
        got, got_s = xd.cpu(), sd.cpu()
        for i, (s, t, n) in enumerate(rows):
            s2 = _next(g, s, t)
            assert int(got_s[i]) == s2, (shape, s, t, n)
            want = torch.where(_banned(g, s2, n), torch.tensor(float("-inf")), x[i, : g.V])
            assert torch.equal(got[i, : g.V].view(I32), want.view(I32)), (shape, s, t, n)
            if s < 0:
                assert torch.equal(got[i].view(I32), x[i].view(I32))
        assert torch.equal(got[:, g.V:].view(I32), x[:, g.V:].view(I32)), shape


# ------------------------------------------------------------------------------------------------ 2. the kernel + the sampler
def test_sampler_behind_the_mask(dev):
    """states OPEN / BODY, n = 3 / 100, T = 0 / 0.7 / 1.5: the token of gr_sample_rows behind the mask is in the allowed set and is
    THE inverse-CDF sample of the float64 softmax over the allowed ids (slack 2e-5: the sampler's own test); greedy rows are the
    arg-max over the allowed ids, first index on ties; top-k alternatives past the allowed set report -inf"""
    from groma_amd import ops
    g, ld = _G(32114, 32004, 32005, 32014, 100, (32008, 32009, 32010, 32011, 32012, 32000)), 32128
    cases = [(s, n, T) for s in (1, 2) for n in (3, 100) for T in (0.0, 0.7, 1.5)]
    R = len(cases)
    x = torch.randn((R, ld), generator=torch.Generator().manual_seed(9)) * 3.0
    x[:, g.V:] = 1e9
    for i, (s, n, T) in enumerate(cases):
        if T == 0.0:                                                        # a tie at the allowed maximum: the first index wins
            x[i, [g.r0 + 1, g.r0 + n - 1]] = 50.0
            x[i, 40] = 60.0                                                 # (and a banned id above it)
    inv = torch.tensor([0.0 if T == 0.0 else 1.0 / T for _, _, T in cases])
    seeds = torch.arange(R, dtype=I64) * 101 + 7
    pos = torch.arange(R, dtype=I32) * 13 + 300
    xd = x.to(dev)
    ops.grammar_step(xd, g.V, torch.tensor([c[0] for c in cases], dtype=I32).to(dev),
                     torch.tensor([c[1] for c in cases], dtype=I32).to(dev), _gids(g))
    out = ops.sample_rows(xd, g.V, inv.to(dev), seeds.to(dev), pos=pos.to(dev), pos_stride=1, pos_off=1).cpu()
    top_ids = torch.full((R, 8), -7, dtype=I64, device=dev)
    top_lp = torch.full((R, 8), 7.0, device=dev)
    out_lp, lp = ops.sample_rows_lp(xd, g.V, inv.to(dev), seeds.to(dev), pos=pos.to(dev), pos_stride=1, pos_off=1,
                                    k=torch.full((R,), 8, dtype=I32, device=dev), top_ids=top_ids, top_lp=top_lp)
    assert torch.equal(out_lp.cpu(), out)
    for i, (s, n, T) in enumerate(cases):
        allowed = (~_banned(g, s, n)).nonzero().flatten()
        assert len(allowed) == n + (1 if s == 2 else 0)
        t = int(out[i])
        assert t in allowed.tolist(), (s, n, T, t)
        xa = x[i, allowed].double()
        if T == 0.0:
            assert t == int(allowed[xa.argmax()]) == g.r0 + 1, (s, n, t)      # (torch.argmax: first maximal index)
        else:
            cdf = torch.cumsum(torch.softmax(xa / T, -1), 0)
            u = ops.sample_uniform(int(seeds[i]), int(pos[i]) + 1)
            j = allowed.tolist().index(t)
            lo = float(cdf[j - 1]) if j > 0 else 0.0
            assert lo - 2e-5 <= u <= float(cdf[j]) + 2e-5, (s, n, T, t, u, lo, float(cdf[j]))
        ref = torch.log_softmax(xa, -1)
        k = min(8, len(allowed))
        tl = top_lp[i].cpu()
        assert set(top_ids[i, :k].tolist()) <= set(allowed.tolist())
        assert float((tl[:k].double() - ref.sort(descending=True).values[:k]).abs().max()) <= 8 * 6.9e-6
        assert bool(torch.isinf(tl[k:]).all()) and bool((tl[k:] < 0).all())
        assert abs(float(lp[i]) - float(ref[allowed.tolist().index(t)])) <= 8 * 6.9e-6


# ------------------------------------------------------------------------------------------------ 3. generate()
N_NEW, EOS = 24, 2


def _run(model, ids, images, graph, seed=11, n=N_NEW, **kw):
    old = model.decode_graph
    model.decode_graph = graph
    try:
        torch.manual_seed(seed)
        return model.generate(ids.clone(), images=images, max_new_tokens=n, return_dict_in_generate=True, output_hidden_states=True, **kw)
    finally:
        model.decode_graph = old


def _n_boxes(out):
    return [int(b.shape[0]) for b in out.hidden_states[0][-1]["pred_boxes"]]


SAMPLE = dict(do_sample=True, temperature=0.9)


@pytest.fixture(scope="module")
def world(dev):
    """the tiny synthetic model with the output-head rows of <roi>, </roi>, the <r_k> and EOS scaled until an UNCONSTRAINED answer
    breaks the grammar within 24 tokens on at least half of 4 rows, greedy and at T = 0.9 (asserted: without it nothing below shows
    anything)"""
    from groma_amd import constants, synth
    cfg, sd, tk = util.tiny_setup(seed=0, max_region_num=37)
    base = cfg.llm_cfg.vocab_size
    special = constants.SyntheticTokenizer().convert_tokens_to_ids(["<roi>", "</roi>"]) + list(tk.box_idx_token_ids)
    images, ids = synth.make_inputs(cfg, tk, bs=4, seed=4321)
    found = None
    for scale in (6.0, 12.0, 24.0, 48.0):
        sd2 = dict(sd)
        extra, head = sd["extra_lm_head.weight"].clone(), sd["llm.lm_head.weight"].clone()
        extra[[t - base for t in special]] *= scale
        head[EOS] *= scale
        sd2["extra_lm_head.weight"], sd2["llm.lm_head.weight"] = extra, head
        model = util.device_model(cfg, sd2)
        model.generation_config.eos_token_id = EOS
        g = _G(cfg.vocab_size, model.bor_token_id, model.eor_token_id, model.box_idx_token_ids[0], len(model.box_idx_token_ids),
               sorted({model.img_token_id, model.reg_token_id, model.refer_box_token_id, model.ground_box_token_id,
                       model.refer_feat_token_id, model.pad_token_id}))
        broken = []
        for kw in ({}, SAMPLE):
            o = _run(model, ids, images, True, **kw)
            new = o.sequences[:, ids.shape[1]:].cpu()
            broken.append(sum(_violation(g, new[b].tolist(), n, EOS) is not None for b, n in enumerate(_n_boxes(o))))
        print(f"\nhead scale {scale}: unconstrained rows that break the grammar: greedy {broken[0]}/4, T=0.9 {broken[1]}/4")
        if min(broken) >= 2:
            found = (cfg, tk, model, g, images, ids)
            break
    assert found is not None, "precondition: no head scale made the unconstrained run break the grammar on half of the rows"
    return found


@pytest.mark.parametrize("sample", [False, True])
def test_generate_grounded_obeys_the_grammar(world, sample):
    cfg, tk, model, g, images, ids = world
    kw = SAMPLE if sample else {}
    P = ids.shape[1]
    outs = {graph: _run(model, ids, images, graph, grounded=True, **kw) for graph in (True, False)}
    o = outs[True]
    new = o.sequences[:, P:].cpu()
    ns = _n_boxes(o)
    assert all(0 < n <= 37 for n in ns)
    for b in range(4):
        assert _violation(g, new[b].tolist(), ns[b], EOS) is None, (b, new[b].tolist())
    assert torch.equal(o.sequences, outs[False].sequences)                  # captured loop == eager loop
    # the grammar is at work, not idle: the constrained answers differ from the unconstrained ones
    plain = _run(model, ids, images, True, **kw)
    assert not torch.equal(plain.sequences[:, : o.sequences.shape[1]], o.sequences[:, : plain.sequences.shape[1]])


def test_generate_grounded_scores_and_logprobs(world):
    """scores are -inf exactly on the banned set of the state the restatement derives from the previous tokens; each token is the
    arg-max of its row; behind <roi> the probabilities of the allowed ids sum to 1 under the kernel's normaliser, within the
    log-probability kernel's own bound (8 x 6.9e-6, profiles/r09_sampler_logprobs.txt)"""
    cfg, tk, model, g, images, ids = world
    P = ids.shape[1]
    outs = {graph: _run(model, ids, images, graph, grounded=True, output_scores=True, output_logprobs=8) for graph in (True, False)}
    o = outs[True]
    ref = _run(model, ids, images, True, grounded=True)
    assert torch.equal(o.sequences, ref.sequences)
    new = o.sequences[:, P:].cpu()
    ns = _n_boxes(o)
    n_open = 0
    for b in range(4):
        states, _ = _states(g, new[b].tolist())
        done = False
        for i, s in enumerate(states):
            row = o.scores[i][b].cpu()
            banned = _banned(g, s, ns[b])
            assert torch.equal(torch.isinf(row) & (row < 0), banned), (b, i, s)
            t = int(new[b, i])
            if not done:
                assert t == int(row.argmax()), (b, i)
                lp = float(o.logprobs[b, i])
                lse = float(row[t]) - lp                                     # the kernel's normaliser
                allowed = (~banned).nonzero().flatten()
                total = float(torch.exp(row[allowed].double() - lse).sum())
                tl, ti = o.top_logprobs[b, i].cpu(), o.top_ids[b, i].cpu()
                k = min(8, len(allowed))
                assert set(ti[:k].tolist()) <= set(allowed.tolist()) and bool(torch.isinf(tl[k:]).all())
                if s == 1:
                    n_open += 1
                    assert len(allowed) == ns[b] and abs(total - 1.0) <= 8 * 6.9e-6, (b, i, total)
            done = done or t == EOS
    assert n_open > 0, "no row opened a region list: the OPEN-step check did not run"
    e = outs[False]
    assert torch.equal(o.logprobs.view(I32), e.logprobs.view(I32)) and torch.equal(o.top_ids, e.top_ids)
    assert all(torch.equal(a.view(I32), b_.view(I32)) for a, b_ in zip(o.scores, e.scores))


@pytest.mark.parametrize("sample", [False, True])
def test_generate_per_row_flags(world, sample):
    """grounded=[True, False, True, False]: the False rows are, token for token, the rows of a plain call under the same seed"""
    cfg, tk, model, g, images, ids = world
    kw = SAMPLE if sample else {}
    P = ids.shape[1]
    plain = _run(model, ids, images, True, **kw).sequences[:, P:].cpu()
    for graph in (True, False):
        o = _run(model, ids, images, graph, grounded=[True, False, True, False], **kw)
        mixed = o.sequences[:, P:].cpu()
        ns = _n_boxes(o)
        m = min(plain.shape[1], mixed.shape[1])
        for b in (1, 3):
            assert torch.equal(mixed[b, :m], plain[b, :m]), (graph, b)
            assert bool((mixed[b, m:] == model.pad_token_id).all()) and bool((plain[b, m:] == model.pad_token_id).all())
        for b in (0, 2):
            assert _violation(g, mixed[b].tolist(), ns[b], EOS) is None, (graph, b)
    with pytest.raises(ValueError):
        model.generate(ids.clone(), images=images, max_new_tokens=2, grounded=[True, False])


# ------------------------------------------------------------------------------------------------ 4. the batcher
@pytest.fixture(scope="module")
def traffic(world):
    from groma_amd import synth
    cfg, tk, model, g, images, ids = world
    gen = torch.Generator().manual_seed(8)
    reqs = []
    for i in range(4):
        img, base = synth.make_inputs(cfg, tk, bs=1, seed=300 + i)
        tail = torch.randint(3, cfg.llm_cfg.vocab_size, (10 + 7 * i,), generator=gen)
        reqs.append(dict(ids=torch.cat([base[0], tail]), image=img[0], seed=40 + i, n=10 + 2 * i,
                         temperature=(0.0, 0.0, 0.8, 0.0)[i], logprobs=(None, None, None, 2)[i]))
    return reqs, {}


def _submit(b, r, grounded):
    return b.submit(r["ids"], r["image"], max_new_tokens=r["n"], seed=r["seed"], temperature=r["temperature"], logprobs=r["logprobs"],
                    **({"grounded": True} if grounded else {}))


def _reference(model, refs, reqs, i, grounded, kw_plain):
    """grounded greedy: generate(grounded=True) of the request alone; grounded sampled: the request alone on a slot batcher (generate
    seeds its sampler from the global RNG, the batcher from the request: their draws differ by design); ungrounded: a batcher built
    WITHOUT the flag"""
    from groma_amd.serving import ContinuousBatcher
    key = (i, grounded, tuple(sorted(kw_plain)) if not grounded else ())
    if key not in refs:
        r = reqs[i]
        if grounded and r["temperature"] == 0.0:
            torch.manual_seed(r["seed"])
            out = model.generate(r["ids"][None].clone(), images=r["image"][None], max_new_tokens=r["n"], grounded=True)
            refs[key] = out[0, r["ids"].shape[0]:].tolist()
        else:
            b = ContinuousBatcher(model, max_rows=4, max_len=1024, **(dict(grounded=True) if grounded else kw_plain))
            rid = _submit(b, r, grounded)
            b.run_until_done()
            assert b.result(rid, pop=False).error is None
            refs[key] = b.result(rid).tokens
    return refs[key]


@pytest.mark.parametrize("mode", ["slots", "prefix"])
def test_batcher_grounded(world, traffic, mode):
    """4 rows, mixed grounded / temperature / logprobs; a second wave with the flags flipped re-uses the slots (prefix mode: hits the
    cache).  Grounded requests equal their reference and obey the grammar, ungrounded ones equal a batcher built without the flag,
    grammar_state is reported, freed slots are unconstrained"""
    from groma_amd.serving import ContinuousBatcher
    cfg, tk, model, g, images, ids = world
    reqs, refs = traffic
    kw = {"slots": {}, "prefix": dict(kv_pages=96, prefix_cache=True)}[mode]
    with pytest.raises(ValueError):
        ContinuousBatcher(model, max_rows=4, max_len=1024, **kw).submit(reqs[0]["ids"], reqs[0]["image"], grounded=True)
    b = ContinuousBatcher(model, max_rows=4, max_len=1024, grounded=True, **kw)
    n_grounded_tokens = 0
    for flags in ([True, False, True, True], [False, True, False, False]):
        rids = [_submit(b, r, f) for r, f in zip(reqs, flags)]
        res = b.run_until_done()
        assert int(b.gstate.max()) == -1                                     # every freed slot is unconstrained again
        for i, (rid, f) in enumerate(zip(rids, flags)):
            r = res[rid]
            assert r.error is None and r.done, r.error
            assert r.tokens == _reference(model, refs, reqs, i, f, kw), (mode, i, f)
            if f:
                n = int(r.pred_boxes.shape[0])
                assert _violation(g, r.tokens, n, EOS) is None, (mode, i, r.tokens)
                assert r.grammar_state == _states(g, r.tokens)[1]
                n_grounded_tokens += len(r.tokens)
            else:
                assert r.grammar_state is None
            if reqs[i]["logprobs"] is not None:
                assert len(r.logprobs) == len(r.tokens) == len(r.top_logprobs) and all(lp <= 0.0 for lp in r.logprobs)
                if f:   # under the constrained distribution: behind <roi> the alternatives are boxes of the image
                    for s, top in zip(_states(g, r.tokens)[0], r.top_logprobs):
                        if s == 1:
                            assert all(g.r0 <= t < g.r0 + n for t, _ in top), top
            b.result(rid)
    assert n_grounded_tokens > 0
    if mode == "prefix":
        assert b.kv_stats()["prefix_hits"] == 4, b.kv_stats()
