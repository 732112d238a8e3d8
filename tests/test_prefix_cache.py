"""Prefix cache of the paged continuous batcher, host side (CPU suite): page reference counts, the prefix key, matching, the page-boundary
rule, LRU eviction, the batcher's argument check, and the argument checks of the two paged prefill entry points (include/groma_hip.h),
which reject before any launch."""
import ctypes

import pytest
import torch

from groma_amd.serving import ContinuousBatcher, PagePool, PrefixCache, prefix_key

P1 = ctypes.c_void_p(1)   # a non-null pointer: validation only, never dereferenced
IMG, REG, PAD = 90, 91, 0


def test_page_pool_retain_release_frees_at_the_last_holder():
    p = PagePool(4)
    a = p.reserve(3)
    p.retain(a[:2])
    p.retain(a[:1])
    assert p.refs(a[0]) == 3 and p.refs(a[1]) == 2 and p.refs(a[2]) == 1 and p.n_shared == 2
    p.release(a)
    assert p.n_free == 2 and p.refs(a[2]) == 0 and p.n_shared == 1    # a[2] went back; a[0], a[1] still held
    p.release(a[:2])
    assert p.n_free == 3 and p.n_shared == 0 and p.refs(a[0]) == 1
    p.release(a[:1])
    assert p.n_free == 4 and p.high_water == 3
    with pytest.raises(ValueError):
        p.retain([a[0]])                      # a free page cannot gain a holder
    with pytest.raises(ValueError):
        p.retain([0])                         # nor can the sink page
    seen = set()
    for _ in range(3):
        ids = p.reserve(4)
        assert 0 not in ids
        seen.update(ids)
        p.retain(ids)
        p.release(ids)
        p.release(ids)
    assert seen == {1, 2, 3, 4} and p.n_free == 4


def test_prefix_key():
    img = torch.randn((3, 8, 8), generator=torch.Generator().manual_seed(0))
    box = torch.tensor([[0.5, 0.5, 0.2, 0.2]])
    k = prefix_key(img, 7, box, None, "bf16")
    assert k == prefix_key(img.clone(), 7, box.clone(), None, "bf16")
    img2 = img.clone()
    img2[0, 0, 0] += 1e-3
    others = [prefix_key(img2, 7, box, None, "bf16"), prefix_key(img, 8, box, None, "bf16"), prefix_key(img, 7, None, None, "bf16"),
              prefix_key(img, 7, None, box, "bf16"), prefix_key(img, 7, box * 2, None, "bf16"), prefix_key(img, 7, box, None, "fp8")]
    assert all(o != k for o in others) and len(set(others)) == len(others)
    assert prefix_key(img, None, box, None, "bf16") is None          # no explicit seed: never shared


def _ids(*parts):
    out = []
    for p in parts:
        out += p.tolist() if isinstance(p, torch.Tensor) else list(p) if isinstance(p, (list, tuple)) else [p]
    return torch.tensor(out, dtype=torch.int64)


def _cache(n_pages=64):
    pool = PagePool(n_pages)
    return pool, PrefixCache(pool, [IMG, REG, PAD])


def _add(cache, pool, key, ids, n_img=100, n_reg=10, e0=None):
    """an entry for un-expanded `ids` whose <image> expands to n_img rows and <region> to 2 * n_reg"""
    L = len(ids) + n_img - 1 + 2 * n_reg - 1
    ids_x = torch.zeros((L,), dtype=torch.int64)
    n_whole = L // 64
    pages = pool.reserve(-(-L // 64))
    e = cache.add(key, ids, ids_x, torch.zeros((1, 4)), pages[:n_whole], None, 64 if e0 is None else e0)
    pool.release(pages)                   # the request that owned them finishes: the entry keeps the whole pages
    return e, L


def test_match_longest_prefix_and_page_boundary():
    pool, c = _cache()
    head = _ids(1, list(range(10, 30)), IMG, list(range(30, 36)), REG)       # 29 ids, placeholders at 21 and 28
    a = _ids(head, list(range(200, 240)))
    e, L = _add(c, pool, "k", a)
    delta = L - len(a)
    assert delta == 99 + 19 and len(e.pages) == L // 64 and pool.n_free == 64 - len(e.pages)
    # shares the head + 5 query ids
    q = _ids(head, list(range(200, 205)), list(range(300, 320)))
    m = c.match("k", q)
    assert m is not None and m.entry is e and m.u == len(head) + 5
    assert m.c == m.u + delta and m.L == m.c + 20 and m.p0 == 64 * (m.c // 64) and m.p0 > 0
    # same key, a longer common prefix in a second entry wins
    b = _ids(head, list(range(200, 230)), list(range(400, 410)))
    e2, _ = _add(c, pool, "k", b)
    m2 = c.match("k", _ids(head, list(range(200, 230)), list(range(400, 406)), 7, 8, 9))
    assert m2.entry is e2 and m2.u == len(head) + 36
    # the same prompt again: p0 stays below L so that the last position is computed
    m3 = c.match("k", a)
    assert m3.c == m3.L == L and m3.p0 == 64 * ((L - 1) // 64) and m3.p0 < L
    # another key never matches
    assert c.match("other", q) is None and c.match(None, q) is None


def test_match_needs_every_placeholder_inside_the_shared_part():
    pool, c = _cache()
    head = _ids(1, list(range(10, 30)), IMG, list(range(30, 36)), REG)
    _add(c, pool, "k", _ids(head, list(range(200, 240))))
    assert c.match("k", _ids(head, 200, 201, IMG, 5)) is None                # an <image> placeholder in the tail
    assert c.match("k", _ids(head, 200, PAD, 5)) is None                     # a pad id in the tail
    assert c.match("k", _ids(1, list(range(10, 30)), IMG, 99, REG, 98)) is None   # diverges before its <region>


def test_match_p0_zero_is_a_miss():
    pool, c = _cache()
    head = _ids(1, IMG, REG)
    # expands to 3 - 2 + 30 + 2 = 33 ... below one page: no whole page, nothing to share
    e, L = _add(c, pool, "k", _ids(head, list(range(50, 80))), n_img=30, n_reg=1, e0=0)
    assert L < 64 and e.pages == []
    assert c.match("k", _ids(head, list(range(50, 60)))) is None
    # an entry of two pages; a request sharing less than a page's worth of expanded positions misses too
    pool2, c2 = _cache()
    e, L = _add(c2, pool2, "k", _ids(head, list(range(50, 150))), n_img=30, n_reg=1, e0=0)
    assert len(e.pages) == L // 64 >= 2
    assert c2.match("k", _ids(head, list(range(50, 60)), 7)) is None         # c = 3 + 10 + 31 = 44 < 64
    m = c2.match("k", _ids(head, list(range(50, 90)), 7))                    # c = 3 + 40 + 31 = 74
    assert m is not None and m.p0 == 64


def test_lru_eviction_order_and_clear():
    pool, c = _cache(8)
    head = _ids(1, IMG, REG)
    ents = [_add(c, pool, f"k{i}", _ids(head, list(range(60, 160))), n_img=30, n_reg=1, e0=0)[0] for i in range(3)]
    assert pool.n_free == 8 - 3 * 2
    c.touch(ents[0])                                                         # k0 used again: k1 is now the oldest
    assert c.evict() and [e.key for e in c.entries.values()] == ["k2", "k0"]
    assert pool.n_free == 4
    held = ents[2].pages
    pool.retain(held)                                                        # a live row maps k2's pages
    assert c.evict() and [e.key for e in c.entries.values()] == ["k0"]
    assert pool.n_free == 4 and all(pool.refs(p) == 1 for p in held)        # still allocated for the row
    pool.release(held)
    assert pool.n_free == 6
    c.clear()
    assert len(c) == 0 and pool.n_free == 8 and not c.evict()


class _Model:
    precision = "bf16"


def test_prefix_cache_needs_kv_pages():
    with pytest.raises(ValueError, match="kv_pages"):
        ContinuousBatcher(_Model(), max_rows=2, max_len=1024, prefix_cache=True)


@pytest.mark.parametrize("precision", ["bf16", "fp16", "ref"])
def test_paged_prefill_entry_points_reject_bad_arguments(precision):
    """null or out-of-range arguments: EINVAL (22) before any launch, in all three builds; the operand-pair build refuses every call"""
    import __graft_entry__ as g
    g.build()
    from groma_amd import _lib
    lib = _lib.load(precision)
    # gr_kv_append_paged(qkv, k_pool, vt_pool, cos, sin, B, H, L, hd, pos0, table, table_ld, pos_dev, pos_stride, stream)
    ka = lib.gr_kv_append_paged
    assert ka(None, P1, P1, None, None, 2, 4, 17, 128, 64, P1, 4, None, 0, None) == 22          # qkv null
    assert ka(P1, P1, P1, None, None, 2, 4, 17, 128, 64, None, 4, None, 0, None) == 22          # table null
    assert ka(P1, P1, P1, P1, None, 2, 4, 17, 128, 64, P1, 4, None, 0, None) == 22              # cos without sin
    assert ka(P1, P1, P1, None, None, 2, 4, 17, 128, 250, P1, 4, None, 0, None) == 22           # pos0 + L > table_ld * 64
    assert ka(P1, P1, P1, None, None, 2, 4, 17, 128, 0, P1, 129, None, 0, None) == 22           # table_ld > 128
    assert ka(P1, P1, P1, None, None, 2, 4, 17, 96, 0, P1, 4, None, 0, None) == 22              # head_dim
    assert ka(P1, P1, P1, None, None, 2, 4, 0, 128, 0, P1, 4, None, 0, None) == 22              # L = 0
    # gr_attention_paged(q, k_pool, vt_pool, out, kv_len, B, H, Lq, table, table_ld, hd, q_pos0, scale, pos_dev, pos_stride, q_ld,
    #                    cos, sin, stream)
    ap = lib.gr_attention_paged
    assert ap(None, P1, P1, P1, None, 2, 4, 17, P1, 4, 128, 64, 1.0, None, 0, 0, None, None, None) == 22    # q null
    assert ap(P1, P1, P1, None, None, 2, 4, 17, P1, 4, 128, 64, 1.0, None, 0, 0, None, None, None) == 22    # out null
    assert ap(P1, P1, P1, P1, None, 2, 4, 17, None, 4, 128, 64, 1.0, None, 0, 0, None, None, None) == 22   # table null
    assert ap(P1, P1, P1, P1, None, 2, 4, 17, P1, 129, 128, 64, 1.0, None, 0, 0, None, None, None) == 22   # > 8192 positions
    assert ap(P1, P1, P1, P1, None, 2, 4, 17, P1, 4, 96, 64, 1.0, None, 0, 0, None, None, None) == 22      # head_dim
    assert ap(P1, P1, P1, P1, None, 2, 4, 17, P1, 4, 128, 250, 1.0, None, 0, 0, None, None, None) == 22    # q_pos0 + Lq > 256
    assert ap(P1, P1, P1, P1, None, 2, 4, 17, P1, 4, 128, 64, 1.0, None, 0, 1540, None, None, None) == 22  # q_ld % 8
    assert ap(P1, P1, P1, P1, None, 2, 4, 17, P1, 4, 128, 64, 1.0, None, 0, 1536, P1, None, None) == 22    # cos without sin
    if precision == "ref":   # no operand-pair form: refused whatever the arguments
        assert ka(P1, P1, P1, None, None, 2, 4, 17, 128, 64, P1, 4, None, 0, None) == 22
        assert ap(P1, P1, P1, P1, None, 2, 4, 17, P1, 4, 128, 64, 1.0, None, 0, 1536, None, None, None) == 22
