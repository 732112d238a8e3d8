"""attention_kernel (slot, paged, operand-pair forms) and decode_attention_kernel against float64, PER OUTPUT ELEMENT, on the mask
and tile edges of tests/attn_cases.py: every case in three score profiles, with finite sentinels in everything the kernel must not
see.  |got - ref| <= (roundings * u + C32) * softmax @ |v| for each element -- the bound tests/test_attn_cases.py proves sound (an
fp32 tile-wise emulation passes it) and biting (an off-by-one limit, a dropped tile-edge key, a q-tile or batch-row mix-up, a missed
rescale, a wrong page are each rejected with a factor >= 2 on every case they apply to).

Each run also checks: the rows before and after `out` (a view into a larger canary-filled buffer) are untouched; two launches over
different canaries give torch.equal results (every row b*Lq + i written, and deterministically)."""
import functools

import pytest
import torch

from tests import attn_cases as A

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in A.CASES}
PAD = 3   # canary rows on either side of `out`


@functools.lru_cache(maxsize=6)
def _dev_data(name, profile, kind):
    """operands built once per (case, profile, kind); the float64 reference is computed on the device"""
    case = BY_NAME[name]
    D = A.make_case(case, profile, kind)
    lim = A.limits(case)
    out, mag = A.ref64(D["q_eff"].cuda(), D["k"].cuda(), D["v"].cuda(), A.visible(lim.cuda(), case.kv_stride), D["scale"])
    return D, out, mag, lim


def _pack(ops, t):
    return (ops.split_pack(t) if ops.SP() == 2 else t.to(ops.H16())).contiguous().cuda()


def _i32(v):
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _guarded(ops, rows, width, run):
    """run(out) twice over different canaries: -> values [rows, width] f32; the guard rows stay, both launches agree bit for bit"""
    res = []
    for canary in (7.0, -3.0):
        buf = torch.full((rows + 2 * PAD, width * ops.SP()), canary, dtype=ops.H16(), device="cuda")
        run(buf[PAD:PAD + rows])
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == canary).all()) and bool((buf[PAD + rows:] == canary).all()), "rows outside `out` were written"
        res.append(buf[PAD:PAD + rows].clone())
    assert torch.equal(res[0], res[1]), "two launches differ (a row left unwritten, or a race)"
    return ops.from_h16(res[0])


def _bhld(x, case):
    return x.view(case.B, case.Lq, case.H, case.hd).permute(0, 2, 1, 3)


def _pos_args(case):
    if case.pos is None:
        return dict(q_pos0=case.q_pos0)
    return dict(pos_dev=_i32(case.pos), pos_stride=case.pos_stride)


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("kind", A.KINDS)
def test_attention_slot(dev, kind, case):
    from groma_amd import ops
    A.check_contract(case)
    with ops.precision(kind):
        for prof in A.PROFILES:
            D, out, mag, lim = _dev_data(case.name, prof, kind)
            k, vt = _pack(ops, D["k"]), _pack(ops, D["v"].transpose(2, 3).contiguous())
            q = _pack(ops, D["qbuf"] if case.fused else D["q"])
            fused = dict(B=case.B, H=case.H, Lq=case.Lq, hd=case.hd, cos=D["cos"].cuda(), sin=D["sin"].cuda()) if case.fused else None
            run = lambda o: ops.attention(q, k, vt, Skv=case.Skv, causal=case.causal, kv_len=_i32(case.kv_len), out=o, fused=fused,
                                          **_pos_args(case))
            got = _guarded(ops, case.B * case.Lq, case.H * case.hd, run)
            A.assert_close(_bhld(got, case), out, mag, kind, case, lim, what=f"attention/{prof}")


@pytest.mark.parametrize("case", [c for c in A.CASES if c.paged], ids=lambda c: c.name)
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_attention_paged(dev, kind, case):
    """gr_attention_paged directly against float64: pages in a random permutation, a sentinel sink page, row 1 mapping row 0's leading
    pages, every row's table shorter than table_ld"""
    from groma_amd import ops
    A.check_contract(case)
    with ops.precision(kind):
        for prof in A.PROFILES:
            D, out, mag, lim = _dev_data(case.name, prof, kind)
            kp, vp, table = A.build_pages(D, case)
            assert int(table.max()) < kp.shape[0] and table.shape[1] == case.table_ld
            kp, vp, table = _pack(ops, kp), _pack(ops, vp), table.cuda()
            q = _pack(ops, D["qbuf"] if case.fused else D["q"])
            rot = dict(cos=D["cos"].cuda(), sin=D["sin"].cuda(), fused=True) if case.fused else {}
            run = lambda o: ops.attention_paged(q, kp, vp, table, B=case.B, H=case.H, Lq=case.Lq, hd=case.hd, kv_len=_i32(case.kv_len),
                                                out=o, **rot, **_pos_args(case))
            got = _guarded(ops, case.B * case.Lq, case.H * case.hd, run)
            A.assert_close(_bhld(got, case), out, mag, kind, case, lim, what=f"attention_paged/{prof}")


@pytest.mark.parametrize("nsplit", [1, 3, None])
@pytest.mark.parametrize("case", [c for c in A.CASES if c.decode], ids=lambda c: c.name)
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_decode_attention_edges(dev, kind, case, nsplit):
    """the Lq = 1 cases through gr_decode_attention and gr_decode_attention_paged: P stays fp32 there, so the bound counts ONE 16-bit
    rounding.  nsplit 3 exceeds the number of 64-key chunks of the short rows (empty slices); a row with no visible key gives zeros,
    merged or not."""
    from groma_amd import ops
    A.check_contract(case)
    HD = case.H * case.hd
    with ops.precision(kind):
        eye = torch.eye(HD, device="cuda").to(ops.H16())
        for prof in A.PROFILES:
            D, out, mag, lim = _dev_data(case.name, prof, kind)
            q, k, vt = _pack(ops, D["q"]), _pack(ops, D["k"]), _pack(ops, D["v"].transpose(2, 3).contiguous())
            kp, vp, table = A.build_pages(D, case)
            kp, vp, table = _pack(ops, kp), _pack(ops, vp), table.cuda()
            smax = case.Skv if case.pos is None else case.kv_stride
            forms = {
                "decode_attention": lambda o: ops.decode_attention(q, k, vt, o, Smax=smax, kv_len=_i32(case.kv_len), nsplit=nsplit,
                                                                   **_pos_args(case)),
                "decode_attention_paged": lambda o: ops.decode_attention_paged(q, kp, vp, o, table, Smax=case.kv_stride,
                                                                               kv_len=_i32(case.kv_len), nsplit=nsplit, **_pos_args(case)),
            }
            for what, fn in forms.items():
                if nsplit == 1:
                    got = _guarded(ops, case.B, HD, fn)
                else:   # key slices: merged by the consumer GEMV's operand load -- an identity weight
                    res = []
                    for _ in range(2):
                        r = fn(torch.empty((case.B, HD), dtype=ops.H16(), device="cuda"))
                        assert isinstance(r, tuple)
                        part, sp = ops.gemv_partials(None, eye, a_parts=r)
                        res.append(part[:sp].sum(0))
                    assert torch.equal(res[0], res[1])
                    got = res[0]
                    fused = torch.full((case.B, HD), 7.0, device="cuda")   # the decode step's own merge (gr_gemv_fused, x_mode 2)
                    ops.gemv_fused(eye, M=case.B, a_parts=r, out=fused)
                    A.assert_close(_bhld(fused, case), out, mag, kind, case, lim, roundings=1, what=f"{what}(nsplit={nsplit})+gemv_fused/{prof}")
                A.assert_close(_bhld(got, case), out, mag, kind, case, lim, roundings=1, what=f"{what}(nsplit={nsplit})/{prof}")
