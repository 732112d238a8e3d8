"""CPU checks of tests/attn_cases.py (the fixtures of tests/test_attention_edges_gpu.py): the bound is sound (a correct fp32
tile-wise kernel with the storage's roundings passes it on every case), it bites (every mutant is rejected, with a factor of 2 to
spare, on every case it applies to), the case list holds every edge it is meant to hold, and every case is inside the kernels'
argument contract.  Also: the KV caches the engine hands to the attention kernels are allocated finite (zeros), which is what lets
attention_kernel feed a visible tile's masked V^T bytes to the MFMA unguarded (include/groma_hip.h, gr_attention_bf16)."""
import functools

import pytest
import torch

from tests import attn_cases as A

BY_NAME = {c.name: c for c in A.CASES}


@functools.lru_cache(maxsize=8)
def _data(name, profile, kind):
    case = BY_NAME[name]
    D = A.make_case(case, profile, kind)
    return D, A.reference(D, case)


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_contract(case):
    A.check_contract(case)
    assert len(BY_NAME) == len(A.CASES)
    for prof in A.PROFILES:     # |score * scale| stays far below the ~200 where fp32 score rounding would matter
        D = A.make_case(case, prof, "bf16")
        s = (D["q_eff"] @ D["k"].double().transpose(-1, -2)).abs().max() * D["scale"]
        assert float(s) < 150.0, (prof, float(s))
        for b in range(case.B):   # sentinels: finite, never zero, and the K sentinel beats every real key of the row
            m = case.kvmax(b)
            if m < case.kv_stride:
                assert float(D["v"][b, :, m:].min()) == A.V_SENTINEL and torch.isfinite(D["k"][b]).all()
                sc = D["q_eff"][b] @ D["k"][b].double().transpose(-1, -2)
                assert m == 0 or float(sc[..., m:].min()) > float(sc[..., :m].max())


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_emulated_kernel_within_bound(case):
    """the fp32 restatement of the algorithm with the storage's roundings of P and of the output passes the comparator"""
    for kind in A.KINDS:
        for prof in A.PROFILES:
            D, (out, mag, lim) = _data(case.name, prof, kind)
            r = A.assert_close(A.emulate(D, case), out, mag, kind, case, lim, what=f"emulated/{prof}")
            assert r <= 1.0


def test_c32_measured():
    """C32 = C32_FACTOR x the fp32 share measured here (the restatement WITHOUT 16-bit roundings against float64) over the whole
    list; it stays a small part of the 16-bit builds' 2u"""
    worst = 0.0
    for case in A.CASES:
        for prof in A.PROFILES:
            D, (out, mag, lim) = _data(case.name, prof, "ref")
            err = (A.emulate(D, case, roundings=False).double() - out).abs()
            ok = mag > 0
            assert float(err[~ok].max() if (~ok).any() else 0.0) == 0.0
            worst = max(worst, float((err[ok] / mag[ok]).max()))
    print(f"fp32 share, worst |emulated - ref64| / mag = {worst:.3e}; C32 = {A.C32:.3e}")
    assert 0.8 * A.C32_MEASURED <= worst <= A.C32_MEASURED, f"measured {worst:.3e}: update C32_MEASURED in tests/attn_cases.py"
    assert A.C32 == A.C32_FACTOR * A.C32_MEASURED and A.C32_FACTOR == 4
    assert A.C32 < 0.02 * 2 * A.U["bf16"] and A.C32 < 0.15 * 2 * A.U["fp16"]


def _verdicts(name):
    """[(case, profile, ratio)] for every case the mutant applies to (bf16 bound: the widest of the three)"""
    fn, profiles = A.MUTANTS[name]
    rows = []
    for case in A.CASES:
        for prof in profiles:
            D, (out, mag, lim) = _data(case.name, prof, "bf16")
            wrong = fn(case, D)
            if wrong is None:
                continue
            rows.append((case, prof, A.compare(wrong, out, mag, "bf16")[0]))
    return rows


@pytest.mark.parametrize("name", list(A.MUTANTS))
def test_comparator_rejects_mutant(name):
    rows = _verdicts(name)
    hit = {c.name for c, _, _ in rows if name not in c.exempt}
    assert len(hit) >= 2, f"{name} applies to {sorted(hit)}: a mutant must apply to at least two cases"
    for case, prof, r in rows:
        print(f"{name:24s} {case.name:18s} {prof:7s} ratio {r:.3g}" + ("  (exempt)" if name in case.exempt else ""))
        if name in case.exempt:
            assert case.exempt[name], "an exemption needs a stated reason"
            continue
        assert r >= 2.0, f"{name} on {case.name}/{prof}: only {r:.3g} x the bound -- the comparator would accept this kernel"
    for case in A.CASES:
        assert set(case.exempt) <= set(A.MUTANTS)


def test_a_noop_mutant_is_noticed(monkeypatch):
    """the sensitivity test fails when a mutant is made a no-op"""
    monkeypatch.setitem(A.MUTANTS, "causal_plus1", (A._limit_mutant(causal_off=0), ("recent",)))
    with pytest.raises(AssertionError):
        test_comparator_rejects_mutant("causal_plus1")


def test_paged_fixture_equals_slot():
    """through the true table a reader sees the slot cache's keys wherever some query looks; everything else holds sentinels"""
    for case in [c for c in A.CASES if c.paged]:
        D = A.make_case(case, "recent", "bf16")
        kp, vp, table = A.build_pages(D, case)
        k1, v1 = A.gather_pages(kp, vp, table, case)
        for b in range(case.B):
            m = case.kvmax(b)
            assert torch.equal(k1[b, :, :m], D["k"][b, :, :m]) and torch.equal(v1[b, :, :m], D["v"][b, :, :m])
            assert float(v1[b, :, m:].min()) == A.V_SENTINEL
            need = -(-(case.pos0(b) + case.Lq) // 64)
            assert int(table[b, need:].abs().max()) == 0 and need < case.table_ld      # the row's table is shorter than table_ld
            assert int(table.max()) < kp.shape[0] and (need == 0 or int(table[b, :need].min()) >= 1)
        used = set(table.flatten().tolist())
        assert float(vp[0].min()) == A.V_SENTINEL and len(set(range(kp.shape[0])) - used) >= 2    # sink + pages in no table


def test_edge_coverage():
    """every edge the list is meant to hold, computed from the list: thinning it later cannot drop one silently"""
    C = A.CASES
    lims = {c.name: A.limits(c) for c in C}
    rows = [(c, b) for c in C for b in range(c.B)]

    def some(pred, what):
        assert any(pred(c) for c in C), f"no case with {what}"

    for hd in (64, 128):
        some(lambda c: c.hd == hd, f"hd {hd}")
    for r in (0, 1, 127):
        some(lambda c: c.Lq % 128 == r and c.Lq > 1, f"Lq % 128 == {r}")
    for L in (1, 15, 16, 17, 32, 33):
        some(lambda c: c.Lq == L, f"Lq == {L}")
    some(lambda c: c.Lq >= 257, "more than one query block plus a one-row block")
    for r in (0, 1, 63):
        some(lambda c: bool(((lims[c.name] % 64 == r) & (lims[c.name] > 0)).any()), f"limit % 64 == {r}")
    for v in (1, 64, 65):
        some(lambda c: bool((lims[c.name] == v).any()), f"limit == {v}")
    for p in (0, 1, 63, 64, 65):
        some(lambda c: c.causal and c.pos is None and c.q_pos0 == p, f"host q_pos0 == {p}")
        some(lambda c: c.pos is not None and p in c.pos, f"pos_dev == {p}")
    some(lambda c: c.causal and c.pos is None and c.q_pos0 > 128, "host q_pos0 > 128")
    some(lambda c: c.pos is not None and max(c.pos) > 128, "pos_dev > 128")
    some(lambda c: c.pos is not None and c.pos_stride == 1 and len(set(c.pos)) > 1, "ragged pos_dev")
    some(lambda c: c.pos is not None and c.pos_stride == 0 and c.B > 1, "a shared pos_dev counter")
    kv = [(c, b, c.kv_len[b]) for c, b in rows if c.kv_len is not None]
    assert any(n == c.skv(b) for c, b, n in kv) and any(n == c.skv(b) - 1 for c, b, n in kv)
    for d in (-1, 0, 1):
        assert any(n > 64 and (n - d) % 64 == 0 for c, b, n in kv), f"no kv_len == 64 m + {d}"
    assert any(n == 1 for c, b, n in kv) and any(n == 0 for c, b, n in kv)
    assert any(c.causal and 0 < n < c.pos0(b) + 1 for c, b, n in kv), "no row whose queries all see the same keys"
    assert any(n == 0 and c.Lq > 1 for c, b, n in kv) and any(n == 0 and c.decode for c, b, n in kv)
    for S in (1, 63, 64, 65, 1025, 582):
        some(lambda c: not c.causal and c.Skv == S, f"non-causal Skv == {S}")
    some(lambda c: c.kv_stride > -(-c.Skv // 64) * 64, "kv_stride > round_up(Skv, 64)")
    some(lambda c: c.Skv % 64 == 0 and c.kv_stride > c.Skv, "a sentinel key right behind a full last tile")
    some(lambda c: c.fused and c.q_ld == 3 * c.H * c.hd, "in-place q")
    some(lambda c: c.fused and c.q_ld > 3 * c.H * c.hd, "in-place q with q_ld > 3*H*hd")
    some(lambda c: c.fused and c.pos is not None and c.pos_stride == 1, "in-place q on ragged rows")
    some(lambda c: c.fused and c.paged and c.hd == 64, "in-place q over pages")
    some(lambda c: c.B == 3 and c.H == 5, "B x H = 3 x 5")
    some(lambda c: c.paged and c.B >= 2 and min(c.kvmax(0), c.kvmax(1)) >= 64, "a row sharing another row's leading pages")
    some(lambda c: c.paged and c.kv_len is not None, "pages + kv_len")
    some(lambda c: c.decode and c.paged and -(-max(c.kvmax(b) for b in range(c.B)) // 64) < 3, "decode with fewer 64-key chunks than nsplit 3")
    assert 25 <= len(C) <= 40


def test_engine_caches_are_allocated_finite():
    """gr_attention_bf16 / gr_attention_paged require finite bytes behind a row's limit in every tile they read: the engine's caches
    start as zeros, growing keeps the prefix and zero-fills the rest, and the 16-bit writers saturate instead of producing inf"""
    from groma_amd import engine, ops
    for prec in ("bf16", "fp16", "ref"):
        with ops.precision(prec):
            c = engine.KVCache(2, 2, 3, 64, 128, "cpu")
            for t in c.k + c.vt:
                assert float(t.float().abs().max()) == 0.0
                t.fill_(1.5)
            c.grow(320)
            for t in c.k:
                assert t.shape[2] == 320 and float(t[:, :, :128].float().min()) == 1.5 and float(t[:, :, 128:].float().abs().max()) == 0.0
            for t in c.vt:
                w = 128 * c.sp
                assert float(t[..., :w].float().min()) == 1.5 and float(t[..., w:].float().abs().max()) == 0.0
    p = engine.PagedKVCache(2, 3, 2, 64, 256, 5, "cpu")
    assert all(float(t.float().abs().max()) == 0.0 for t in p.k + p.vt) and int(p.table.abs().max()) == 0
