"""Paged KV cache, host side (CPU suite): the page bookkeeping of the continuous batcher and the argument checks of the paged entry
points (include/groma_hip.h), which reject before any launch."""
import ctypes

import pytest

from groma_amd.serving import PagePool

P1 = ctypes.c_void_p(1)   # a non-null pointer: validation only, never dereferenced


def test_page_pool_reserve_release_and_high_water():
    p = PagePool(5)
    assert p.n_free == 5 and p.high_water == 0
    a = p.reserve(2)
    b = p.reserve(3)
    assert len(a) == 2 and len(b) == 3 and not set(a) & set(b)
    assert sorted(a + b) == [1, 2, 3, 4, 5]          # page 0 is the sink page: never handed out
    assert p.n_free == 0 and p.high_water == 5
    assert p.reserve(1) is None and p.n_free == 0    # exhausted: nothing taken
    assert p.reserve(0) == []
    p.release(a)
    assert p.n_free == 2 and p.high_water == 5
    c = p.reserve(2)
    assert sorted(c) == sorted(a)                    # freed pages are handed out again
    p.release(b)
    p.release(c)
    assert p.n_free == 5 and p.high_water == 5


def test_page_pool_refuses_bad_releases():
    p = PagePool(3)
    a = p.reserve(2)
    p.release(a[:1])
    with pytest.raises(ValueError):
        p.release(a[:1])                             # double release
    with pytest.raises(ValueError):
        p.release([0])                               # the sink page is never in use
    with pytest.raises(ValueError):
        p.release([a[1], a[1]])                      # the same page twice in one call
    assert p.n_free == 2                             # a refused release changes nothing
    with pytest.raises(ValueError):
        PagePool(0)


def test_page_pool_never_hands_out_the_sink_page():
    p = PagePool(64)
    seen = set()
    for _ in range(10):
        ids = p.reserve(64)
        assert ids is not None and 0 not in ids
        seen.update(ids)
        p.release(ids[::-1])
    assert seen == set(range(1, 65))


def _gemv_desc(_lib):
    d = _lib.GemvDesc()
    d.W, d.q, d.kc, d.vt = 1, 1, 1, 1
    d.M, d.N, d.K, d.ldw = 4, 3 * 4 * 128, 512, 512
    d.x_mode, d.h, d.ldh, d.gamma, d.eps = 1, 1, 512, 1, 1e-5
    d.epi, d.H, d.HD, d.kv_stride, d.pos0 = 3, 4, 128, 1024, 0
    return d


@pytest.mark.parametrize("precision", ["bf16", "fp16", "ref"])
def test_paged_entry_points_reject_bad_arguments(precision):
    """null or out-of-range arguments: EINVAL (22) before any launch, in all three builds"""
    import __graft_entry__ as g
    g.build()
    from groma_amd import _lib
    lib = _lib.load(precision)
    # gr_decode_attention_paged(q, k_pool, vt_pool, out, kv_len, B, H, Smax, table, table_ld, hd, q_pos0, scale, pos_dev, pos_stride,
    #                           nsplit, parts, stream)
    da = lib.gr_decode_attention_paged
    assert da(None, P1, P1, P1, None, 1, 4, 64, P1, 1, 128, 0, 1.0, None, 0, 1, None, None) == 22          # q null
    assert da(P1, P1, P1, P1, None, 1, 4, 64, None, 1, 128, 0, 1.0, None, 0, 1, None, None) == 22          # table null
    assert da(P1, P1, P1, P1, None, 1, 4, 128, P1, 1, 128, 0, 1.0, None, 0, 1, None, None) == 22          # Smax > table_ld * 64
    assert da(P1, P1, P1, P1, None, 1, 4, 8192, P1, 129, 128, 0, 1.0, None, 0, 1, None, None) == 22       # table_ld > 128
    assert da(P1, P1, P1, P1, None, 1, 4, 64, P1, 1, 96, 0, 1.0, None, 0, 1, None, None) == 22             # head_dim
    assert da(P1, P1, P1, P1, None, 1, 4, 64, P1, 1, 128, 0, 1.0, None, 0, 2, None, None) == 22            # nsplit > 1, no parts
    assert da(P1, P1, P1, P1, None, 1, 4, 64, P1, 1, 128, 64, 1.0, None, 0, 1, None, None) == 22           # q_pos0 past Smax
    # gr_qkv_split_paged(qkv, q, k_pool, vt_pool, cos, sin, B, H, L, hd, pos0, table, table_ld, pos_dev, pos_stride, stream)
    qs = lib.gr_qkv_split_paged
    assert qs(None, P1, P1, P1, None, None, 1, 4, 1, 128, 0, P1, 2, None, 0, None) == 22                   # qkv null
    assert qs(P1, P1, P1, P1, None, None, 1, 4, 2, 128, 0, P1, 2, None, 0, None) == 22                     # L != 1
    assert qs(P1, P1, P1, P1, None, None, 1, 4, 1, 128, 0, None, 2, None, 0, None) == 22                   # table null
    assert qs(P1, P1, P1, P1, P1, None, 1, 4, 1, 128, 0, P1, 2, None, 0, None) == 22                       # cos without sin
    assert qs(P1, P1, P1, P1, None, None, 1, 4, 1, 128, 128, P1, 2, None, 0, None) == 22                   # pos0 past the table
    # gr_kv_scatter_pages(k_src, vt_src, k_pool, vt_pool, table, table_ld, src_rows, dst_rows, lens, n, n_src, n_dst, H, S, hd,
    #                     max_len, stream)
    ks = lib.gr_kv_scatter_pages
    assert ks(None, P1, P1, P1, P1, 2, P1, P1, P1, 1, 1, 1, 4, 128, 128, 128, None) == 22                  # k_src null
    assert ks(P1, P1, P1, P1, P1, 2, P1, None, P1, 1, 1, 1, 4, 128, 128, 128, None) == 22                  # dst_rows null
    assert ks(P1, P1, P1, P1, P1, 2, P1, P1, P1, 1, 1, 1, 4, 100, 128, 100, None) == 22                    # S % 64
    assert ks(P1, P1, P1, P1, P1, 2, P1, P1, P1, 1, 1, 1, 4, 256, 128, 192, None) == 22                    # max_len > table_ld * 64
    assert ks(P1, P1, P1, P1, P1, 2, P1, P1, P1, 1, 1, 1, 4, 128, 128, 192, None) == 22                    # max_len > S
    assert ks(P1, P1, P1, P1, P1, 2, P1, P1, P1, 0, 1, 1, 4, 128, 128, 128, None) == 22                    # n = 0
    # gr_gemv_fused_paged(desc, table, table_ld, stream)
    gp = lib.gr_gemv_fused_paged
    d = _gemv_desc(_lib)
    assert gp(None, P1, 2, None) == 22
    assert gp(ctypes.byref(d), None, 2, None) == 22                                                       # table null
    assert gp(ctypes.byref(d), P1, 0, None) == 22                                                         # table_ld
    assert gp(ctypes.byref(d), P1, 129, None) == 22
    d.epi, d.C, d.ldc = 0, 1, d.N
    assert gp(ctypes.byref(d), P1, 2, None) == 22                                                         # not the QKV epilogue
    d = _gemv_desc(_lib)
    d.M = 9
    assert gp(ctypes.byref(d), P1, 2, None) == 22                                                         # > 8 rows


def test_split_build_has_no_paged_form():
    """libgroma_hip_ref.so: every paged entry point returns EINVAL on any call, also a well-formed one"""
    from groma_amd import _lib
    lib = _lib.load("ref")
    assert lib.gr_decode_attention_paged(P1, P1, P1, P1, None, 1, 4, 64, P1, 1, 128, 0, 1.0, None, 0, 1, None, None) == 22
    assert lib.gr_qkv_split_paged(P1, P1, P1, P1, None, None, 1, 4, 1, 128, 0, P1, 1, None, 0, None) == 22
    assert lib.gr_kv_scatter_pages(P1, P1, P1, P1, P1, 2, P1, P1, P1, 1, 1, 1, 4, 128, 128, 128, None) == 22
    assert lib.gr_gemv_fused_paged(ctypes.byref(_gemv_desc(_lib)), P1, 2, None) == 22
