"""Teacher-forced scoring on the GPU: gr_label_logprob_rows against the CPU, then GromaModel.score() on the tiny model.

Exact parts are torch.equal.  logprob and lse are compared with float64 under a bound that is derived, not chosen: the error a
float32 numpy restatement of the kernel's formula in the kernel's documented summation order (csrc/score.hip) makes against
float64 on the same entries, times 8 for the device's few-ulp exp / log (`_measure`)."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

F32 = np.float32
NINF = F32(-np.inf)
IG = -100
T, WAVES = 256, 4  # threads of a workgroup, its waves


# ------------------------------------------------------------------------------------------------ CPU restatement
def _exp(a):
    return np.exp(a.astype(F32)).astype(F32)


def _unit(m, s, v):
    """one unit (v [T, N]: a 16-byte vector, or one tail element) into every thread's state, as score_unit does"""
    u = v.max(axis=1)
    up = u > m
    s = np.where(up, (s * _exp(m - u)).astype(F32), s)
    m = np.where(up, u, m)
    live = m > NINF
    for e in range(v.shape[1]):
        s = np.where(live, (s + _exp(v[:, e] - m)).astype(F32), s)
    return m, s


def _f(a, M):
    return np.where(a == NINF, F32(0), _exp(a - M))


def _merge(m, s, om, os_):
    M = np.maximum(m, om)
    return M, ((s * _f(m, M)).astype(F32) + (os_ * _f(om, M)).astype(F32)).astype(F32)


def _lse_f32(x):
    """gr_label_logprob_rows' log-normaliser of one row in numpy float32, in the kernel's order: thread tid takes the 16-byte vectors
    tid, tid + 256, ... (online maximum + rescaled sum, the four elements added in index order), then one of the V % 4 tail
    elements; the wave butterfly (lane ^ 32, 16, 8, 4, 2, 1); the four wave leaders merged in wave order; lse = m + log(s)."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=F32)
        V = x.shape[0]
        nv = V // 4
        n_it = -(-nv // T)
        xv = np.full((n_it * T, 4), NINF, dtype=F32)   # (a unit past the last vector is -inf in the kernel too: it adds exactly 0)
        xv[:nv] = x[: 4 * nv].reshape(nv, 4)
        m, s = np.full(T, NINF, dtype=F32), np.zeros(T, dtype=F32)
        for it in range(n_it):
            m, s = _unit(m, s, xv[it * T: (it + 1) * T])
        tail = np.full((T, 1), NINF, dtype=F32)
        tail[: V - 4 * nv, 0] = x[4 * nv:]
        if V > 4 * nv:
            m, s = _unit(m, s, tail)
        m, s = m.reshape(WAVES, 64), s.reshape(WAVES, 64)
        o = 32
        while o > 0:
            idx = np.arange(64) ^ o
            m, s = _merge(m, s, m[:, idx], s[:, idx])
            o >>= 1
        am, as_ = m[0, 0], s[0, 0]
        for w in range(1, WAVES):
            am, as_ = _merge(am, as_, m[w, 0], s[w, 0])
        return F32(am + F32(np.log(F32(as_))))


# ------------------------------------------------------------------------------------------------ the kernel's input set
def _cases():
    """(name, x [rows, ld] f32, V, labels [rows] i64, misaligned): every input the issue lists; columns V..ld hold 1e30"""
    g = torch.Generator().manual_seed(2024)
    out = []
    V = 32128
    x = torch.randn((12, V + 8), generator=g) * 3.0
    lab = torch.zeros(12, dtype=torch.int64)
    x[0, [5, 17000, 32127]] = x[0, :V].max() + 1.0                  # exact ties at the maximum: the first index wins; label 0
    lab[0] = 0
    x[1, [100, 1023, 31000]] = 2.5                                  # ties at the label's value on both sides of it; the label is
    lab[1] = 1023                                                   # the last element of the block's first stride (256 x 4 ids)
    x[2, :V] = torch.randn((V,), generator=g)                       # one dominant logit: every other exp underflows to 0
    x[2, 12345] = 200.0
    lab[2] = 3                                                      # the last id of 16-byte vector 0
    x[3, :V] = torch.randn((V,), generator=g)
    x[3, 1024] = 200.0                                              # the dominant logit IS the label, first id of the second stride
    lab[3] = 1024
    x[4, :V] = (torch.randn((V,), generator=g) * 2.0).round()       # a row of a few distinct values (ties everywhere)
    lab[4] = 4                                                      # the first id of 16-byte vector 1
    x[5, :V] = float("-inf")                                        # -inf over most ids (a grammar-masked row), the label allowed
    x[5, 29000:29010] = torch.randn((10,), generator=g)
    lab[5] = 29003
    x[6, 100:20000] = float("-inf")                                 # the label sits on -inf
    lab[6] = 150
    x[7, :V] = float("-inf")                                        # an all -inf row
    lab[7] = 10
    x[8] = float("nan")                                             # two ignored rows: never read
    x[9] = float("nan")
    lab[8] = lab[9] = IG
    lab[10] = V                                                     # a label one past the vocabulary
    lab[11] = V - 1
    x[:, V:] = 1e30
    out.append(("V32128", x, V, lab, False))
    for V in (5000, 1000, 37):                                      # V = 37, ld = 61: rows 1, 2, 3, 5 are not 16-byte aligned
        x = torch.randn((6, V + 24), generator=g) * 2.0
        x[0, [V - 1, 3]] = x[0, :V].max() + 2.0
        x[:, V:] = 1e30
        out.append((f"V{V}", x, V, torch.tensor([3, V - 1, 0, V // 2, 4, V - 2]), False))
    name, x, V, lab, _ = out[1]
    out.append(("V5000-misaligned", x, V, lab, True))               # the same rows at a base 4 bytes off: the scalar path, same bits
    V = 1000                                                        # more rows than the chip has CUs
    x = torch.randn((300, V + 24), generator=g) * 2.5
    x[:, V:] = 1e30
    out.append(("rows300", x, V, torch.randint(0, V, (300,), generator=g), False))
    return out


def _run_kernel(x, V, lab, misaligned=False):
    from groma_amd import ops
    rows, ld = x.shape
    if misaligned:
        store = torch.full((rows * ld + 4,), 1e30, device="cuda")
        xd = store[1: 1 + rows * ld].view(rows, ld)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    else:
        xd = x.cuda()
    lp, lse, greedy, rank = ops.label_logprob_rows(xd, V, lab.cuda(), lse=True, greedy=True, rank=True)
    torch.cuda.synchronize()
    return dict(lp=lp.cpu(), lse=lse.cpu(), greedy=greedy.cpu(), rank=rank.cpu())


def _same(a, b):
    """float64 comparison of two [n] vectors: -inf / NaN by equality, the largest difference of the rest"""
    a, b = a.double(), b.double()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~fin & ~torch.isnan(b)], b[~fin & ~torch.isnan(b)]), (a, b)
    assert bool(torch.isfinite(a[fin]).all())
    return float((a[fin] - b[fin]).abs().max()) if bool(fin.any()) else 0.0


_MEASURED = {}


def _measure():
    """the module's one measurement: the kernel on every row of _cases() -> (runs, bound, float32 error, device error).  Entries:
    logprob and lse of every row that is not ignored (nothing skipped or filtered); the label = V row has its lse only."""
    if not _MEASURED:
        cases = _cases()
        runs = {name: _run_kernel(x, V, lab, mis) for name, x, V, lab, mis in cases}
        e32 = worst = 0.0
        for name, x, V, lab, _ in cases:
            r = runs[name]
            keep = (lab >= 0).nonzero().flatten().tolist()
            xs = x[keep, :V]
            ref_lse = torch.logsumexp(xs.double(), -1)
            ref_lp = torch.log_softmax(xs.double(), -1)
            t = lab[keep].clamp(max=V - 1)
            ref_lp = ref_lp[torch.arange(len(keep)), t]
            ref_lp[lab[keep] >= V] = float("nan")
            with np.errstate(all="ignore"):
                my_lse = torch.from_numpy(np.array([_lse_f32(xs[i].numpy()) for i in range(len(keep))], dtype=F32))
                my_lp = torch.from_numpy((xs[torch.arange(len(keep)), t].numpy() - my_lse.numpy()).astype(F32))
            my_lp[lab[keep] >= V] = float("nan")
            e32 = max(e32, _same(my_lse, ref_lse), _same(my_lp, ref_lp))
            worst = max(worst, _same(r["lse"][keep], ref_lse), _same(r["lp"][keep], ref_lp))
        _MEASURED.update(runs=runs, tol=8.0 * e32, e32=e32, dev=worst)
    return _MEASURED["runs"], _MEASURED["tol"], _MEASURED["e32"], _MEASURED["dev"]


# ------------------------------------------------------------------------------------------------ the kernel
def test_kernel_exact_parts(dev):
    """greedy == the first index of a stable descending sort, rank == the label's place in it; an ignored row gives exactly
    0.0 / 0.0 / -1 / -1 (its NaN logits are not read); label = V gives NaN / -1 with lse and greedy as usual; the 1e30 behind V is
    never read; a misaligned base gives the aligned run's bits; two runs give the same bits"""
    runs = _measure()[0]
    for name, x, V, lab, mis in _cases():
        r = runs[name]
        for row in range(x.shape[0]):
            t = int(lab[row])
            if t < 0:
                assert float(r["lp"][row]) == 0.0 and float(r["lse"][row]) == 0.0, (name, row)
                assert int(r["greedy"][row]) == -1 and int(r["rank"][row]) == -1, (name, row)
                continue
            order = torch.sort(x[row, :V], descending=True, stable=True).indices
            assert int(r["greedy"][row]) == int(order[0]), (name, row)
            if t >= V:
                assert bool(torch.isnan(r["lp"][row])) and int(r["rank"][row]) == -1, (name, row)
                assert bool(torch.isfinite(r["lse"][row])), (name, row)
            else:
                assert int(r["rank"][row]) == int((order == t).nonzero()[0]), (name, row)
        again = _run_kernel(x, V, lab, mis)
        for key in ("lp", "lse", "greedy", "rank"):
            a, b = r[key], again[key]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (name, key)
    big = runs["V32128"]
    assert int(big["greedy"][0]) == 5 and int(big["rank"][1]) == int((_cases()[0][1][1, :32128] > 2.5).sum()) + 1
    assert int(big["greedy"][7]) == 0 and int(big["rank"][7]) == 10 and bool(torch.isnan(big["lp"][7])) and float(big["lse"][7]) == float("-inf")
    assert float(big["lp"][6]) == float("-inf") and int(big["rank"][3]) == 0
    for key in ("lp", "lse", "greedy", "rank"):                      # the scalar path: same units, same order, same bits
        a, b = runs["V5000"][key], runs["V5000-misaligned"][key]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), key


def test_kernel_optional_outputs_and_argument_checks(dev):
    """logprob alone == logprob with every output asked for; the wrapper checks dtypes and one label per row"""
    from groma_amd import ops
    name, x, V, lab, _ = _cases()[2]
    alone = ops.label_logprob_rows(x.cuda(), V, lab.cuda())
    assert isinstance(alone, torch.Tensor) and torch.equal(alone.cpu().view(torch.int32), _measure()[0][name]["lp"].view(torch.int32))
    rank = torch.full((6,), 77, dtype=torch.int32, device="cuda")
    lp = ops.label_logprob_rows(x.cuda(), V, lab.cuda(), rank=rank)[0]
    assert torch.equal(rank.cpu(), _measure()[0][name]["rank"]) and torch.equal(lp.cpu().view(torch.int32), alone.cpu().view(torch.int32))
    with pytest.raises(ValueError):
        ops.label_logprob_rows(x.cuda(), V, lab[:-1].cuda())
    with pytest.raises(TypeError):
        ops.label_logprob_rows(x.cuda(), V, lab.int().cuda())
    with pytest.raises(TypeError):
        ops.label_logprob_rows(x.double().cuda(), V, lab.cuda())
    with pytest.raises(RuntimeError):
        ops.label_logprob_rows(x.cuda(), x.shape[1] + 1, lab.cuda())   # ld < V: EINVAL from the C entry


def test_kernel_against_float64(dev):
    """logprob and lse of EVERY non-ignored row of the input set against torch.log_softmax / logsumexp in float64.
    Bound = 8 x the float32 restatement's own maximum error on the same entries (_measure).
    Measured on an MI355X: float32 restatement 1.393e-06 -> bound 1.114e-05; device 1.393e-06."""
    _, tol, e32, worst = _measure()
    print(f"\nlabel logprob / lse error vs float64: float32 restatement {e32:.3e} -> bound {tol:.3e}; device {worst:.3e}")
    assert e32 > 0.0 and worst <= tol, (worst, tol)


# ------------------------------------------------------------------------------------------------ score()
def _inputs(cfg, tk):
    from groma_amd import synth
    images, ids = synth.make_inputs(cfg, tk, bs=3, seed=1234)
    labels = torch.full_like(ids, IG)
    labels[0, -5:] = ids[0, -5:]                                     # the last 5 prompt tokens of row 0
    reg = int((ids[1] == tk.reg_token_id).nonzero()[0])
    pos1 = [2, 19, 25, reg + 1, 40, 41, 77, 100, ids.shape[1] - 1]  # 9 scattered tokens of row 1, one right behind <region>
    labels[1, pos1] = ids[1, pos1]
    return images, ids, labels, pos1                                 # (nothing on row 2)


def _expanded(model, ids, pred_boxes, b, c):
    """expanded position of the caller's position c of row b: <image> becomes n_img_tok rows, <region> two per selected box"""
    img = int((ids[b] == model.img_token_id).nonzero()[0])
    reg = int((ids[b] == model.reg_token_id).nonzero()[0])
    n_img = (model.vit.G // 2) ** 2
    return c + (n_img - 1 if c > img else 0) + (2 * pred_boxes[b].shape[0] - 1 if c > reg else 0)


def _score(model, ids, labels, images, seed=5, **kw):
    torch.manual_seed(seed)   # (the region shuffle draws from the CPU generator: the same seed, the same regions)
    return model.score(ids.clone(), labels.clone(), images=images, **kw)


def _check_own_logits(out, targets, tol):
    """a ScoreOutput against its own logits: log-probabilities within the kernel bound of float64 log_softmax, greedy ids and ranks
    equal to a stable sort"""
    lp, rank, greedy = torch.cat(out.token_logprobs), torch.cat(out.token_ranks), torch.cat(out.greedy_ids)
    lg = out.logits.cpu()
    assert lg.shape[0] == lp.numel() == targets.numel() and lg.dtype == torch.float32
    ref = torch.log_softmax(lg.double(), -1)[torch.arange(lp.numel()), targets]
    err = float((lp.double() - ref).abs().max())
    assert err <= tol, (err, tol)
    order = torch.sort(lg, dim=-1, descending=True, stable=True).indices
    assert torch.equal(greedy, order[:, 0])
    assert torch.equal(rank.long(), (order == targets[:, None]).long().argmax(-1))
    return err


def _check_model(model, cfg, tk, check_loss):
    tol = _measure()[1]
    images, ids, labels, pos1 = _inputs(cfg, tk)
    V = cfg.vocab_size
    torch.manual_seed(5)
    before = model.generate(ids.clone(), images=images, max_new_tokens=4)
    out = _score(model, ids, labels, images, return_logits=True)
    torch.manual_seed(5)
    after = model.generate(ids.clone(), images=images, max_new_tokens=4)
    assert torch.equal(before, after)                                # the shared arenas are not disturbed
    torch.manual_seed(5)
    fwd = model.forward(input_ids=ids.clone(), labels=labels.clone(), images=images, return_dict=True)
    assert all(torch.equal(a, b) for a, b in zip(out.pred_boxes, fwd.hidden_states[1]["pred_boxes"]))
    # bookkeeping
    P = ids.shape[1]
    assert out.num_tokens.tolist() == [5, 9, 0] and out.num_tokens.dtype == torch.int64
    assert out.positions[0].tolist() == list(range(P - 5, P)) and out.positions[1].tolist() == pos1 and out.positions[2].numel() == 0
    targets = torch.cat([labels[b, out.positions[b]] for b in range(3)])
    assert torch.equal(targets, torch.cat([ids[b, out.positions[b]] for b in range(3)]))
    for name, dt in (("token_logprobs", torch.float32), ("token_ranks", torch.int32), ("greedy_ids", torch.int64)):
        vals = getattr(out, name)
        assert [int(v.numel()) for v in vals] == [5, 9, 0] and all(v.dtype == dt and v.dim() == 1 for v in vals), name
    assert out.logits.shape == (14, V)
    # the logits of the scored rows are forward's logits one expanded position in front of each label
    rows = [(b, _expanded(model, ids, out.pred_boxes, b, int(c)) - 1) for b in range(3) for c in out.positions[b]]
    want = torch.stack([fwd.logits[b, p] for b, p in rows])
    assert util.relerr(out.logits, want) < 1e-5, util.relerr(out.logits, want)
    _check_own_logits(out, targets, tol)
    # sums and the loss
    seq = torch.stack([v.double().sum() for v in out.token_logprobs])
    assert out.sequence_logprob.dtype == torch.float64 and torch.equal(out.sequence_logprob, seq) and float(seq[2]) == 0.0
    assert abs(float(out.loss) - float(-seq.sum() / 14)) <= 1e-12 * abs(float(out.loss))
    if check_loss:
        assert abs(float(out.loss) - float(fwd.loss)) <= 1e-5 * abs(float(fwd.loss)), (float(out.loss), float(fwd.loss))
    plain = _score(model, ids, labels, images)
    assert plain.logits is None and torch.equal(torch.cat(plain.token_logprobs).view(torch.int32), torch.cat(out.token_logprobs).view(torch.int32))
    return out, targets, tol, (images, ids, labels, pos1)


@pytest.fixture(scope="module")
def tiny(dev):
    cfg, sd, tk = util.tiny_setup(seed=0)
    model = util.device_model(cfg, sd)
    model.generation_config.eos_token_id = None
    return cfg, sd, tk, model


def test_score_matches_forward(tiny):
    cfg, sd, tk, model = tiny
    _check_model(model, cfg, tk, check_loss=True)


def test_score_head_chunks_and_batching(tiny):
    """head_rows 3 / 8 / 2048: the same logits within one GEMM's tile-choice bound, each run inside the kernel bound of its own
    logits; row 1 alone meets the bounds the batch of three meets"""
    cfg, sd, tk, model = tiny
    tol = _measure()[1]
    images, ids, labels, pos1 = _inputs(cfg, tk)
    targets = torch.cat([ids[0, -5:], ids[1, pos1]])
    outs = {hr: _score(model, ids, labels, images, return_logits=True, head_rows=hr) for hr in (3, 8, 2048)}
    for hr, o in outs.items():
        assert o.num_tokens.tolist() == [5, 9, 0], hr
        _check_own_logits(o, targets, tol)
        assert util.relerr(o.logits, outs[2048].logits) < 1e-5, hr
    with pytest.raises(ValueError):
        model.score(ids.clone(), labels.clone(), images=images, head_rows=0)
    alone = _score(model, ids[1:2], labels[1:2], images[1:2], return_logits=True)
    assert alone.num_tokens.tolist() == [9] and alone.positions[0].tolist() == pos1
    _check_own_logits(alone, ids[1, pos1], tol)
    torch.manual_seed(5)
    fwd = model.forward(input_ids=ids[1:2].clone(), labels=labels[1:2].clone(), images=images[1:2], return_dict=True)
    want = torch.stack([fwd.logits[0, _expanded(model, ids[1:2], alone.pred_boxes, 0, c) - 1] for c in pos1])
    assert util.relerr(alone.logits, want) < 1e-5
    assert abs(float(alone.loss) - float(fwd.loss)) <= 1e-5 * abs(float(fwd.loss))


def test_score_nothing_and_bad_labels(tiny):
    cfg, sd, tk, model = tiny
    images, ids, labels, pos1 = _inputs(cfg, tk)
    none = _score(model, ids, torch.full_like(ids, IG), images, return_logits=True)
    assert none.num_tokens.tolist() == [0, 0, 0] and bool(torch.isnan(none.loss)) and none.sequence_logprob.tolist() == [0.0] * 3
    assert none.logits is None and len(none.pred_boxes) == 3 and all(v.numel() == 0 for v in none.token_logprobs)
    first = torch.full_like(ids, IG)
    first[:, 0] = ids[:, 0]                                          # only first labels: never scored
    assert _score(model, ids, first, images).num_tokens.tolist() == [0, 0, 0]
    bad = labels.clone()
    bad[1, 40] = cfg.vocab_size
    with pytest.raises(ValueError):
        model.score(ids.clone(), bad, images=images)
    with pytest.raises(ValueError):
        model.score(ids.clone(), labels[:, :-1].clone(), images=images)


def test_score_ground_box_label(tiny):
    """a label on a <ground_box> placeholder: the scored target is the matched <r_k> id, and the caller's labels (and input_ids) are
    rewritten in place as forward does"""
    cfg, sd, tk, model = tiny
    images, ids, labels, pos1 = _inputs(cfg, tk)
    ids = ids.clone()
    ids[0, 42] = tk.ground_box_token_id
    lab = torch.full_like(ids, IG)
    lab[0, 42], lab[0, 43] = ids[0, 42], ids[0, 43]
    ground = [torch.tensor([[0.7, 0.6, 0.25, 0.3]]), torch.empty((0, 4)), torch.empty((0, 4))]
    ids_a, lab_a = ids.clone(), lab.clone()
    torch.manual_seed(5)
    out = model.score(ids_a, lab_a, images=images, ground_boxes=ground, return_logits=True)
    ids_b, lab_b = ids.clone(), lab.clone()
    torch.manual_seed(5)
    fwd = model.forward(input_ids=ids_b, labels=lab_b, images=images, ground_boxes=ground, return_dict=True)
    assert int(lab_a[0, 42]) in tk.box_idx_token_ids and torch.equal(lab_a, lab_b) and torch.equal(ids_a, ids_b)
    assert int(ids_a[0, 42]) == int(lab_a[0, 42])
    assert out.num_tokens.tolist() == [2, 0, 0] and out.positions[0].tolist() == [42, 43]
    targets = lab_a[0, [42, 43]]
    _check_own_logits(out, targets, _measure()[1])
    assert abs(float(out.loss) - float(fwd.loss)) <= 1e-5 * abs(float(fwd.loss))


@pytest.mark.parametrize("kind", ["hybrid-fp16", "fp8"])
def test_score_other_precisions(dev, kind):
    from groma_amd import constants
    from groma_amd.groma import GromaModel
    cfg, sd, tk = util.tiny_setup(seed=0)
    kw = dict(fp8=True) if kind == "fp8" else dict(precision=kind)
    model = GromaModel.from_state_dict(cfg, sd, "cuda", **kw)
    model.init_special_token_id(constants.SyntheticTokenizer())
    model.generation_config.eos_token_id = None
    _check_model(model, cfg, tk, check_loss=False)
